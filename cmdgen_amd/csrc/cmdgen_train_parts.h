// cmdgen_train_parts.h - the parts several of the training step's kernels are composed of (kernels_train_gemm.hip, kernels_train_dgrad.hip,
// and the scalar helpers every training unit uses).  Device code only.  Every part is short straight-line code; none asks which kernel it is
// in.  What differs between the kernels that share a part enters as a template parameter or a small callable:
//   dst(c)          the weight-gradient staging: where the eight k values of channel c go (the 128-tile kernel swizzles there);
//   add(t)          the partial reductions: where a workgroup's slice sum is added.
// The kernels keep their names, signatures, launch bounds and LDS; a part repeats the expressions and sum orders of the bodies it replaces.
// (Pieces only one kernel family uses stay beside it: the training GEMM's staging and body in kernels_train_gemm.hip.)
#pragma once
#include "cmdgen_dev.h"
#include "cmdgen_split.h"
#include "cmdgen_train_kernels.h"
#include "cmdgen_wlayout.h"

// ---------------------------------------------------------------------------------------------------------------- scalars
__device__ __forceinline__ float silu_exact(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float dsilu(float v) {            // d/dv v*sigmoid(v) = s * (1 + v * (1 - s))
    const float s = sigmoid_f(v);        // v_exp_f32 + v_rcp_f32 (2 ulp), the forward's own sigmoid: expf + an IEEE division
                                         // cost ~25 instructions per element in every dgrad epilogue
    return s * (1.0f + v * (1.0f - s));
}
__device__ __forceinline__ float4 silu4(const float4& v) { return make_float4(silu_f(v.x), silu_f(v.y), silu_f(v.z), silu_f(v.w)); }
__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- weight-gradient staging
// A staging thread of k_wgrad_split / k_wgrad_split128 holds eight consecutive k rows of four channels, v[8].  (A pointer, not a reference to
// the array: with the reference the one-piece kernels kept v in scratch.)
__device__ __forceinline__ void wg_fetch8(float4* v /* [8] */, const float* gsrc, int ld, int k_first, int k_end) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = k_first + i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < k_end) v[i] = *reinterpret_cast<const float4*>(gsrc + (size_t)k * ld);
    }
}
__device__ __forceinline__ void wg_silu8(float4* v /* [8] */) {        // X_p holds pre-activations (WgradBatch::xs)
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = silu4(v[i]);
}
__device__ __forceinline__ void wg_colsum8(float4& colsum, const float4* v /* [8] */) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { colsum.x += v[i].x; colsum.y += v[i].y; colsum.z += v[i].z; colsum.w += v[i].w; }
}
// the eight k values of one channel, split into the NPC pieces (1: the leading bf16 piece only): one 16-byte store per plane, the planes PE
// elements apart
template <int NPC>
__device__ __forceinline__ void wg_store_octet(unsigned short* d, int PE, float k0, float k1, float k2, float k3, float k4, float k5, float k6, float k7) {
    if constexpr (NPC == 3) {
        sbf16x8 p0, p1, p2;
        split8(make_float4(k0, k1, k2, k3), make_float4(k4, k5, k6, k7), p0, p1, p2);
        *reinterpret_cast<sbf16x8*>(d) = p0; *reinterpret_cast<sbf16x8*>(d + PE) = p1; *reinterpret_cast<sbf16x8*>(d + 2 * PE) = p2;
    } else {
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        const u4 q = {cvt_pk_bf16(k0, k1), cvt_pk_bf16(k2, k3), cvt_pk_bf16(k4, k5), cvt_pk_bf16(k6, k7)};
        *reinterpret_cast<u4*>(d) = q;
    }
}
// transpose in registers: channel c gets the eight k values v[0..7].c; dst(c) = where channel c's octet lies in plane 0
template <int NPC, class DST>
__device__ __forceinline__ void wg_stage8(const float4* v /* [8] */, int PE, DST dst) {
    wg_store_octet<NPC>(dst(0), PE, v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x);
    wg_store_octet<NPC>(dst(1), PE, v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y);
    wg_store_octet<NPC>(dst(2), PE, v[0].z, v[1].z, v[2].z, v[3].z, v[4].z, v[5].z, v[6].z, v[7].z);
    wg_store_octet<NPC>(dst(3), PE, v[0].w, v[1].w, v[2].w, v[3].w, v[4].w, v[5].w, v[6].w, v[7].w);
}
// the products of one 16-k step over MM x NN accumulators: small terms first, every product exact in fp32; each (a piece, b piece) pair
// runs over all accumulators before the next pair
template <int NPC, int MM, int NN>
__device__ __forceinline__ void split_mfmas(f32x16 (&acc)[MM][NN], const sbf16x8 (&a)[MM][NPC], const sbf16x8 (&b)[NN][NPC]) {
    auto products = [&](int ai, int bi) {
#pragma unroll
        for (int m = 0; m < MM; ++m)
#pragma unroll
            for (int n = 0; n < NN; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][ai], b[n][bi], acc[m][n], 0, 0, 0);
    };
    if constexpr (NPC == 3) { products(2, 0); products(1, 1); products(0, 2); products(1, 0); products(0, 1); }
    products(0, 0);
}

// ---------------------------------------------------------------------------------------------------------------- gate / head
// adjoint of k_coord_out + coord2diff for edge e: given dacc [N][4] (gradient of the per-node coordinate sums),
//   dphi = (cd . dacc[row]) * range * (1 - tanh^2 phi);  dcd = g * dacc[row]
// writes dcd_out[e] and returns dphi
__device__ __forceinline__ float coord_out_edge(const CoordOutArgs& co, int e) {
    const int i = co.row[e], j = co.col[e];
    const float4 a = co.X[i], b = co.X[j];
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    const float r = dx * dx + dy * dy + dz * dz;
    const float den = sqrtf(r + 1e-8f) + co.norm_constant;
    const float cx = dx / den, cy = dy / den, cz = dz / den;
    const float4 dv = *reinterpret_cast<const float4*>(co.dacc + (size_t)i * 4);
    const float dd = co.adiv ? co.adiv[i] : co.dacc_div;          // aggregation 'mean': the receiver's edge count (egnn_new.py:288-292), else normalization_factor
    const float da[3] = {dv.x / dd, dv.y / dd, dv.z / dd};      // dL/d acc = dL/dx_{l+1} / divisor
    const float p = co.phi[e];
    const float th = co.use_tanh ? tanhf(p) : 0.f;
    const float g = co.use_tanh ? th * co.range : p;
    const float dg = cx * da[0] + cy * da[1] + cz * da[2];
    co.dcd_out[e] = make_float4(g * da[0], g * da[1], g * da[2], 0.f);
    return co.use_tanh ? dg * co.range * (1.0f - th * th) : dg;
}

// ---------------------------------------------------------------------------------------------------------------- partial reductions
// One slice-and-sum: the workgroup sums rows w = slice's share of [0, nwg) of src[w * stride + off] - four rows in flight per column, 64
// columns per workgroup, `on`: this thread's column exists - and its first wave hands the total to add(t): one atomic per column and slice.
template <class ADD>
__device__ __forceinline__ void reduce_slice(int nwg, int nslices, int slice, const float* src, size_t stride, size_t off, bool on, ADD add) {
    __shared__ float red[4][64];
    const int part = threadIdx.x >> 6;
    const int per = (nwg + nslices - 1) / nslices;
    const int w0 = slice * per, w1 = min(nwg, w0 + per);
    float sum = 0.f;
    if (on) {
#pragma unroll 4
        for (int w = w0 + part; w < w1; w += 4) sum += src[(size_t)w * stride + off];
    }
    red[part][threadIdx.x & 63] = sum;
    __syncthreads();
    if (part == 0 && on) add((red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]));
}
