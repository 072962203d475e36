"""The arithmetic of the matrix engines, emulated on the CPU, and its accuracy on a [2048, 256] x [256, 256] product of SiLU activations and uniform
weights (run as a script): the fp32 fmaf chain / BLAS sgemm the reference runs, the three-piece bf16 split (six MFMAs per product) and the half
engine (two fp16 pieces, three MFMAs; weights times 1024) - each against the float64 product.  DESIGN.md section 4a-v quotes these numbers.

The emulation: an operand is split into pieces by rounding and subtracting (split); a product is the listed piece pairs, smallest first, per 16-wide
k block, with the products inside an MFMA exact and ONE fp32 rounding of the accumulator per MFMA (mfma_sum).  tests/f64_ref.py imports ENGINES,
split and mfma_sum from here for its CPU models of the engines, so the tool and the tests state one arithmetic."""
import numpy as np
import torch

KB = 16                     # k extent of one emulated MFMA
HALF_SCALE = 1024.0         # the half engine multiplies the weights by this before it splits them, and the result by its inverse
# engine -> (pieces per operand, the rounding that forms a piece, (activation piece, weight piece) of every product in issue order, weight scale)
ENGINES = {
    'half': (2, torch.float16, ((1, 0), (0, 1), (0, 0)), HALF_SCALE),
    'bf3': (3, torch.bfloat16, ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)), 1.0),
}


def split(x, n, to):
    """fp32 tensor -> n fp32 tensors, each exactly representable in `to`: piece k is the rounding of what pieces 0..k-1 leave."""
    out, r = [], x.to(torch.float32)
    for _ in range(n):
        p = r.to(to).to(torch.float32)
        out.append(p)
        r = r - p
    return out


def mfma_sum(a_pieces, w_pieces, pairs):
    """sum over k blocks and `pairs` of a_pieces[i][:, block] @ w_pieces[j][block]: every MFMA's 16 products exact (float64), the fp32 accumulator
    rounded once per MFMA.  a_pieces [M, K], w_pieces [K, N]; K is padded with zeros to a multiple of 16."""
    M, K = a_pieces[0].shape
    N = w_pieces[0].shape[1]
    nb = (K + KB - 1) // KB
    pad = nb * KB - K
    # [nb, M, 16] and [nb, 16, N], float64
    A = [torch.nn.functional.pad(a, (0, pad)).to(torch.float64).reshape(M, nb, KB).permute(1, 0, 2).contiguous() for a in a_pieces]
    W = [torch.nn.functional.pad(w, (0, 0, 0, pad)).to(torch.float64).reshape(nb, KB, N) for w in w_pieces]
    acc, acc64, part = torch.zeros((M, N), dtype=torch.float32), torch.empty((M, N), dtype=torch.float64), torch.empty((M, N), dtype=torch.float64)
    for kb in range(nb):
        for i, j in pairs:
            torch.mm(A[i][kb], W[j][kb], out=part)      # one MFMA's products, exact
            torch.add(part, acc, out=acc64)
            acc.copy_(acc64)                            # ... and the one rounding of its accumulator
    return acc


def engine_product(a, w, engine, omit=None):
    """a [M, K] @ w [K, N] (fp32 tensors) as `engine` computes it; omit = one (activation piece, weight piece) pair left out (a planted defect)."""
    n, to, pairs, scale = ENGINES[engine]
    r = mfma_sum(split(a, n, to), split(w * scale, n, to), [p for p in pairs if p != omit])
    return r / scale if scale != 1.0 else r


def main():
    rng = np.random.default_rng(0)
    M, K, N = 2048, 256, 256
    pre = rng.normal(0, 1.5, size=(M, K)).astype(np.float32)
    A = (pre / (1 + np.exp(-pre))).astype(np.float32)
    W = rng.uniform(-1 / 16, 1 / 16, size=(K, N)).astype(np.float32)
    exact = A.astype(np.float64) @ W.astype(np.float64)
    At, Wt = torch.from_numpy(A), torch.from_numpy(W)
    r_bf = engine_product(At, Wt, 'bf3').numpy()
    r_h = engine_product(At, Wt, 'half').numpy()
    acc = np.zeros((M, N), np.float32)
    for k in range(K):
        acc = (acc.astype(np.float64) + A[:, k:k + 1].astype(np.float64) * W[k:k + 1].astype(np.float64)).astype(np.float32)
    for name, r in (('fp32 fmaf chain', acc), ('BLAS sgemm', A @ W), ('bf16 x 3, six products', r_bf), ('fp16 x 2, three products (half engine)', r_h)):
        e = r.astype(np.float64) - exact
        print(f'{name:42s} rms error {np.sqrt((e ** 2).mean()):.3e}   max {np.abs(e).max():.3e}   (rms of the result {np.sqrt((exact ** 2).mean()):.3f})')


if __name__ == '__main__':
    main()
