// cmdgen_sampler.h - device helpers of the conditional sampler kernels (kernels_ddpm.hip, kernels_inpaint.hip, kernels_score.hip, kernels_multi.hip).
// These translation units are built with -ffp-contract=off, so the same helper rounds the same way in each.
#pragma once
#include "cmdgen_dev.h"
#include "cmdgen_launch.h"

__device__ __forceinline__ void atomic_max_pos(unsigned int* slot, float v) {
    atomicMax(slot, __float_as_uint(fabsf(v)) & 0x7fffffffu);     // non-negative floats order like their bits (a NaN's sign bit is cleared: any NaN ranks above +Inf)
}

// max that keeps a NaN (fmaxf drops it): torch's x.abs().max() returns NaN as soon as one element is NaN, and the
// reference's assertion then fails (NaN < 1e-2 is False) - so a NaN must survive into the recorded maxima
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? __uint_as_float(0x7fc00000u) : fmaxf(a, b); }

// records the two maxima assert_mean_zero_with_mask compares (en_diffusion.py:919-924).  Non-negative floats order like
// their bits and the quiet NaN 0x7fc00000 lies above +Inf, so atomicMax on the bits keeps a NaN once one sample has it.
__device__ __forceinline__ void record_com_check(unsigned int* slot2, const float* zx, int ld, int pb,
                                                 int nl, float scale, int lane) {
    float mx = 0.f;
    for (int i = lane; i < nl; i += 64) {
        const float* p = zx + (size_t)(pb + i) * ld;
        mx = max_nan(mx, max_nan(fabsf(p[0] * scale), max_nan(fabsf(p[1] * scale), fabsf(p[2] * scale))));
    }
    for (int o = 32; o > 0; o >>= 1) mx = max_nan(mx, __shfl_xor(mx, o));
    float s = 0.f;
    if (lane < 3) for (int i = 0; i < nl; ++i) s += zx[(size_t)(pb + i) * ld + lane] * scale;
    s = fabsf(s);
    s = max_nan(s, max_nan(__shfl(s, 1), __shfl(s, 2)));
    if (lane == 0) { atomic_max_pos(slot2, mx); atomic_max_pos(slot2 + 1, s); }
}
