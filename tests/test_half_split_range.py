"""The low end of the half matrix engine's range, emulated on the CPU (no GPU needed).

The half engine (cmdgen_split.h) splits an fp32 operand into two fp16 pieces, a0 = fp16(a) and a1 = fp16(a - a0), and a product into
a1 b0 + a0 b1 + a0 b0, each exact in the fp32 accumulator.  Weights are pre-multiplied by a power of two (WPack::wh_scale) so their pieces
stay normal; activations are not.  Below 2^-3 an activation's second piece is an fp16 subnormal, and a row whose activations are all that
small loses accuracy against its own result, the more the smaller they are.  The library flags rows whose max |a| lies below HALF_LOW_TAU
and runs them on the bf16 split engine; this test restates the split in numpy and checks that rows at or above the threshold stay well
inside the evaluation tolerance and that rows far below it do not.
"""
import numpy as np

from helpers import tau_from_header

K = 256
EVAL_TOL = 2e-5          # the evaluation tolerance of the GPU tests (helpers.EVAL_TOL)


def half_pieces(x):
    x = np.asarray(x, np.float32)
    x0 = x.astype(np.float16)
    x1 = (x - x0.astype(np.float32)).astype(np.float16)        # the difference is exact in fp32
    return x0.astype(np.float32), x1.astype(np.float32)


def half_engine_gemm(a, w):
    """a [M, K] x w[N, K]^T as the half engine computes it: scaled weight pieces, three products summed in fp32."""
    sc = np.float32(2.0 ** (11 - np.floor(np.log2(np.abs(w).max()))))      # largest weight in [2^11, 2^12)
    w0, w1 = half_pieces(w * sc)
    a0, a1 = half_pieces(a)
    acc = (a1 @ w0.T).astype(np.float32)
    acc = (acc + (a0 @ w1.T)).astype(np.float32)
    acc = (acc + (a0 @ w0.T)).astype(np.float32)
    return acc / sc


def worst_row_error(got, a, w):
    """max over rows of the row's max error relative to the row's largest exact result"""
    exact = a.astype(np.float64) @ w.astype(np.float64).T
    err = np.abs(got.astype(np.float64) - exact).max(axis=1)
    return float((err / np.abs(exact).max(axis=1)).max())


def silu_rows(rng, rows, row_max):
    """SiLU activations of N(0, 2) pre-activations, each row scaled so that its max |a| is row_max"""
    x = rng.normal(0.0, 2.0, (rows, K))
    a = x / (1.0 + np.exp(-x))
    a *= row_max / np.abs(a).max(axis=1, keepdims=True)
    return a.astype(np.float32)


def errors_at(row_max, seed=0):
    rng = np.random.default_rng(seed)
    w = (rng.normal(0.0, 1.0, (K, K)) / np.sqrt(K)).astype(np.float32)
    a = silu_rows(rng, 256, row_max)
    sgemm = worst_row_error((a @ w.T).astype(np.float32), a, w)
    half = worst_row_error(half_engine_gemm(a, w), a, w)
    return half, sgemm


def test_threshold_is_a_power_of_two_below_the_subnormal_edge():
    tau = tau_from_header()
    assert tau == 2.0 ** round(np.log2(tau)) and tau <= 2.0 ** -3


def test_rows_at_or_above_the_threshold_stay_inside_the_tolerance():
    """From tau up a row's worst error stays below half the evaluation tolerance (within 1.5x an fp32 sgemm from 2^-2 up)."""
    tau = tau_from_header()
    for seed in (0, 1):
        for row_max in (tau, 2 * tau, 4 * tau, 0.125, 1.0, 4.0):
            half, sgemm = errors_at(row_max, seed)
            assert half <= EVAL_TOL / 2, f'rows with max |a| = {row_max}: half engine {half:.2e} > {EVAL_TOL / 2:.1e}'
            if row_max >= 0.25:
                assert half <= 1.5 * sgemm, f'rows with max |a| = {row_max}: half engine {half:.2e} > 1.5 x sgemm {sgemm:.2e}'


def test_rows_far_below_the_threshold_leave_the_tolerance():
    """At tau / 16 the error exceeds the evaluation tolerance (and any sgemm bound): why such rows are flagged and re-run."""
    tau = tau_from_header()
    half, sgemm = errors_at(tau / 16)
    assert half > EVAL_TOL and half > 10 * sgemm, f'rows with max |a| = tau / 16: half engine {half:.2e}, sgemm {sgemm:.2e}'
