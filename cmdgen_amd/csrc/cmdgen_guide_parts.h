// cmdgen_guide_parts.h - the parts the guided chains' kernels share (kernels_restrain.hip, kernels_diverse.hip): the wave reductions, the
// denoised estimate, the frame shift, the clip of a displacement and what an op of the diverse chain runs for a sample.  Device code only; every unit that includes this is built with
// -ffp-contract=off.  The expressions and sum orders are those the restrained chains' bit-for-bit tests pin.
#pragma once
#include "cmdgen_step_parts.h"

__device__ __forceinline__ float wave_sum(float v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ float wave_max(float v) { for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return v; }

// com of the np positions s_q[0 .. np-1] (one wave; every lane returns it)
__device__ __forceinline__ void wave_com(const float4* s_q, int np, int lane, float& c0, float& c1, float& c2) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int a = lane; a < np; a += 64) { const float4 p = s_q[a]; a0 += p.x; a1 += p.y; a2 += p.z; }
    const float cnt = fmaxf((float)np, 1.0f);
    c0 = wave_sum(a0) / cnt; c1 = wave_sum(a1) / cnt; c2 = wave_sum(a2) / cnt;
}

// xhat of a free row, one x column, in Angstrom: the denoised estimate from z and the network's column e (zero when the NaN guard reset);
// sa: the op's guide row (sigma_t, alpha_t, 0, 0)
__device__ __forceinline__ float xhat_free(const Dims& d, const float4& sa, float z, float e, bool nan_reset) {
    if (nan_reset) e = 0.f;
    return d.norm_x * (z - sa.x * e) / sa.y;
}

// shift = n_x (com(P.x) - com(P_in.x / n_x)), by one wave, from sample b's np pocket atoms in LDS -> s_shift; gb: the chain's guide buffer
// (RestrainBuf, DiverseBuf), whose pin_com k_restrain_prep filled
template <class GuideBuf>
__device__ __forceinline__ void frame_shift(const Dims& d, const GuideBuf& gb, int b, const float4* s_q, int np, int lane, float* s_shift) {
    float c0, c1, c2;
    wave_com(s_q, np, lane, c0, c1, c2);
    const float4 pin = gb.pin_com[b];
    if (lane == 0) { s_shift[0] = d.norm_x * (c0 - pin.x); s_shift[1] = d.norm_x * (c1 - pin.y); s_shift[2] = d.norm_x * (c2 - pin.z); }
}

// a displacement longer than max_shift is scaled back to it
__device__ __forceinline__ void clip_shift(float max_shift, float& dx, float& dy, float& dz) {
    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
    if (len > max_shift) { const float f = max_shift / len; dx *= f; dy *= f; dz *= f; }
}

// what an op of the diverse chain runs for sample b: guided - the displacement enters the mean; terms - steps 1-3 of kernels_diverse.hip run at all
// (for the displacement, or for op_overlap alone).  Uniform over the workgroup, and the same in all three launches of the op.
struct DiverseOp { bool guided, terms; };
__device__ __forceinline__ DiverseOp diverse_op(const DiverseBuf& db, int b, const float4& cf) {
    const bool coupled = db.set_size[b] > 1;
    const bool guided = coupled && db.strength > 0.f && cf.w <= db.guide_below;
    return DiverseOp{guided, coupled && (guided || db.op_overlap != nullptr)};
}
