"""Cases, inputs and reference results of the multi-pocket scoring tests (test_hip_multi_score.py on the GPU, test_multi_score_cpu.py
without one): multi_pocket_cases' MIXED, LARGE and PAIRS pockets, weights and config; K = 5 levels plus t = 0 (200, 400, .., 1000, 0
at T = 1000); given rows drawn per case with PCG64(first_index + 7) - normal(0, 2 A) positions, uniform types; noise
torch.randn((6, Nu, 11)) seeded first_index + 1.  The reference is multi_score_ref.score_levels, live, fp32 on the CPU, computed once
per case and shared.  A (level, group) entry is left out of a parity comparison when any member's inputs hold a pair within
multi_score_ref.BAND of the cutoff - at most multi_score_ref.CAP of a case's entries, from the inputs alone (test_multi_score_cpu.py
asserts it; none is left out in these three cases)."""
import numpy as np
import torch

import multi_pocket_cases as mc
import multi_pocket_ref as mp
import multi_score_ref as ms
import score_ref
from multi_pocket_cases import CASES, LARGE, MIXED, PAIRS, config, member_pockets, params, pocket_dict, state_dict, weights_of  # noqa: F401

K = 5
_REF = {}


def levels():
    return score_ref.level_list(config().timesteps, K)


def given_rows(case):
    """(x [Nu, 3], one_hot [Nu, 8]) float32: the groups' given pharmacophores in the pockets' common frame."""
    nu = int(sum(case.nph))
    rng = np.random.Generator(np.random.PCG64(case.first_index + 7))
    x = rng.normal(0.0, 2.0, size=(nu, 3)).astype(np.float32)
    types = rng.integers(0, 8, size=nu)
    return x, np.eye(8, dtype=np.float32)[types]


def noise_of(case):
    return torch.randn((K + 1, int(sum(case.nph)), 11), generator=torch.Generator().manual_seed(case.first_index + 1))


def reference(case):
    """dict(pb, weights, noise, groups, x, one_hot, levels, raw) - raw: multi_score_ref.score_levels' dict; computed once."""
    if case.name not in _REF:
        torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
        pb, w, noise = member_pockets(case), weights_of(case), noise_of(case)
        groups = mp.Groups(case.group_sizes, case.nph)
        x, oh = given_rows(case)
        with torch.no_grad():
            raw = ms.score_levels(params(), config().as_dict(), groups, x, oh, pocket_dict(pb), w, levels(), noise)
        _REF[case.name] = dict(pb=pb, weights=w, noise=noise, groups=groups, x=x, one_hot=oh, levels=levels(), raw=raw)
    return _REF[case.name]
