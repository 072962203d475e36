"""Geometric restraints of the restrained sampling chain (ConditionalDDPM.sample_restrained, cmdgen_restrained_chain): the list-of-dicts
form the Python entry points take, its validation, and the record array the library reads.  Pure numpy: nothing here needs a device.

A restraint is a dict:
  {'kind': 'position',  'sample': b, 'point': i, 'center': (x, y, z), 'radius': r, 'k': k}     point i within r of the centre
  {'kind': 'distance',  'sample': b, 'points': (i, j), 'lo': lo, 'hi': hi, 'k': k}             points i and j between lo and hi apart
  {'kind': 'exclusion', 'sample': b, 'center': (x, y, z), 'radius': r, 'k': k}                 no point of the sample within r of the centre
Lengths in Angstrom, k in 1/Angstrom^2, centres in the frame of the pocket the chain is given.  The energy of a restraint is 0.5 k v^2 with
v its violation (the header of csrc/kernels_restrain.hip has the definition)."""
import math

import numpy as np

KINDS = {'position': 0, 'distance': 1, 'exclusion': 2}          # include/cmdgen_hip.h: CMDGEN_RESTRAINT_*
MAX_RESTRAINTS = 256                                            # per sample (CMDGEN_MAX_RESTRAINTS)
DEFAULT_MAX_SHIFT = 1.0                                         # A per op and point ("Restrained sampling": how it was chosen)
DEFAULT_CLASH_K = 1.0

# cmdgen_restraint
RESTRAINT_DTYPE = np.dtype([('kind', np.int32), ('sample', np.int32), ('i', np.int32), ('j', np.int32), ('c', np.float32, (3,)),
                            ('a', np.float32), ('b', np.float32), ('k', np.float32)])
assert RESTRAINT_DTYPE.itemsize == 40

_KEYS = {'position': {'kind', 'sample', 'point', 'center', 'radius', 'k'},
         'distance': {'kind', 'sample', 'points', 'lo', 'hi', 'k'},
         'exclusion': {'kind', 'sample', 'center', 'radius', 'k'}}


def _bad(n, r, why):
    return ValueError(f'restraints[{n}] = {r!r}: {why}')


def _nonneg(n, r, key):
    try:
        v = float(r[key])
    except (TypeError, ValueError):
        raise _bad(n, r, f'{key} is not a number') from None
    if not math.isfinite(v) or v < 0.0:
        raise _bad(n, r, f'{key}={v} must be finite and >= 0')
    return v


def _center(n, r):
    try:
        c = [float(v) for v in r['center']]
    except (TypeError, ValueError):
        raise _bad(n, r, 'center is not three numbers') from None
    if len(c) != 3 or not all(math.isfinite(v) for v in c):
        raise _bad(n, r, 'center must be three finite numbers')
    return c


def _point(n, r, v, nl, sample, owner='sample'):
    if isinstance(v, bool) or int(v) != v:
        raise _bad(n, r, f'point index {v!r} is not an integer')
    if not 0 <= int(v) < nl:
        raise _bad(n, r, f'point {int(v)}: {owner} {sample} has {nl} points')
    return int(v)


def records(restraints, num_phar, sample=None, owner='sample'):
    """The checked record array (RESTRAINT_DTYPE) of a list of restraint dicts.  num_phar [B]: points per sample.  sample: None - every
    dict names its 'sample'; an int - the dicts carry none and all belong to that sample.  owner: what a 'sample' is called in the messages
    ('group' where the records belong to the groups of a multi-pocket call).  ValueError names the offending entry."""
    nph = np.asarray(num_phar, dtype=np.int64).reshape(-1)
    out = np.zeros(len(restraints), dtype=RESTRAINT_DTYPE)
    per_sample = np.zeros(len(nph), dtype=np.int64)
    for n, r in enumerate(restraints):
        if not isinstance(r, dict) or 'kind' not in r:
            raise _bad(n, r, "expected a dict with a 'kind'")
        kind = r['kind']
        if kind not in KINDS:
            raise _bad(n, r, f'unknown kind {kind!r}: expected one of {sorted(KINDS)}')
        keys = set(_KEYS[kind]) - ({'sample'} if sample is not None else set())
        if set(r) != keys:
            missing, extra = sorted(keys - set(r)), sorted(set(r) - keys)
            raise _bad(n, r, f"a '{kind}' restraint has the keys {sorted(keys)}" + (f'; missing {missing}' if missing else '') +
                       (f'; not understood {extra}' if extra else ''))
        b = r['sample'] if sample is None else sample
        if isinstance(b, bool) or int(b) != b or not 0 <= int(b) < len(nph):
            raise _bad(n, r, f'{owner} {b!r} outside the batch of {len(nph)} {owner}s')
        b, nl = int(b), int(nph[int(b)])
        rec = out[n]
        rec['kind'], rec['sample'], rec['k'] = KINDS[kind], b, _nonneg(n, r, 'k')
        if kind == 'distance':
            pts = r['points']
            if not hasattr(pts, '__len__') or len(pts) != 2:
                raise _bad(n, r, 'points must be a pair (i, j)')
            rec['i'], rec['j'] = _point(n, r, pts[0], nl, b, owner), _point(n, r, pts[1], nl, b, owner)
            if rec['i'] == rec['j']:
                raise _bad(n, r, f"a distance between point {int(rec['i'])} and itself (i == j)")
            lo, hi = _nonneg(n, r, 'lo'), _nonneg(n, r, 'hi')
            if lo > hi:
                raise _bad(n, r, f'lo={lo} > hi={hi}')
            rec['a'], rec['b'] = lo, hi
        else:
            if kind == 'position':
                rec['i'] = _point(n, r, r['point'], nl, b, owner)
            rec['c'] = _center(n, r)
            rec['a'] = _nonneg(n, r, 'radius')
        per_sample[b] += 1
        if per_sample[b] > MAX_RESTRAINTS:
            raise _bad(n, r, f'{owner} {b} has more than {MAX_RESTRAINTS} restraints')
    return out


def clash_pair(clash):
    """clash: None (off), a radius, or (radius, k) -> (radius, k) checked."""
    if clash is None:
        return 0.0, 0.0
    r, k = (clash, DEFAULT_CLASH_K) if isinstance(clash, (int, float)) else tuple(clash)
    r, k = float(r), float(k)
    if not (math.isfinite(r) and math.isfinite(k)) or r < 0.0 or k < 0.0:
        raise ValueError(f'clash={clash!r}: the radius and k must be finite and >= 0')
    return r, k


def check_scalars(scale, max_shift, guide_below):
    scale, max_shift, guide_below = float(scale), float(max_shift), float(guide_below)
    if not math.isfinite(scale) or scale < 0.0:
        raise ValueError(f'scale={scale} must be finite and >= 0')
    if not math.isfinite(max_shift) or max_shift <= 0.0:
        raise ValueError(f'max_shift={max_shift} must be finite and > 0')
    if not 0.0 <= guide_below <= 1.0:
        raise ValueError(f'guide_below={guide_below} must be in [0, 1]')
    return scale, max_shift, guide_below


# ---- diverse sampling (ConditionalDDPM.sample_diverse): its scalar and partition checks live beside check_scalars
MAX_SET_ROWS = 8192                  # = CMDGEN_MAX_SET_ROWS (include/cmdgen_hip.h): phar rows of one set


def check_diverse_scalars(strength, width, max_shift, guide_below):
    """The scalars of diverse sampling (ConditionalDDPM.sample_diverse, cmdgen_diverse_chain), checked as check_scalars checks its own."""
    strength, width = float(strength), float(width)
    if not math.isfinite(strength) or strength < 0.0:
        raise ValueError(f'strength={strength} must be finite and >= 0')
    if not math.isfinite(width) or width <= 0.0:
        raise ValueError(f'width={width} must be finite and > 0')
    _, max_shift, guide_below = check_scalars(0.0, max_shift, guide_below)
    return strength, width, max_shift, guide_below


def check_set_sizes(set_sizes, num_nodes_phar):
    """set_sizes: the samples partitioned into sets of consecutive samples -> int64 array [S], checked against num_nodes_phar [B]."""
    nph = np.asarray(num_nodes_phar, dtype=np.int64).reshape(-1)
    raw = np.asarray(set_sizes).reshape(-1)
    if len(raw) < 1 or not np.all(np.isfinite(raw.astype(np.float64))) or np.any(raw != np.floor(raw)):
        raise ValueError(f'set_sizes={list(raw)}: expected at least one integer size')
    sizes = raw.astype(np.int64)
    if np.any(sizes < 1):
        raise ValueError(f'set_sizes={sizes.tolist()}: every set has at least one sample')
    if int(sizes.sum()) != len(nph):
        raise ValueError(f'set_sizes sums to {int(sizes.sum())}, the batch has {len(nph)} samples')
    rows = np.add.reduceat(nph, np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    if np.any(rows > MAX_SET_ROWS):
        raise ValueError(f'set_sizes: set {int(np.argmax(rows))} has {int(rows.max())} phar rows, at most {MAX_SET_ROWS}')
    return sizes
