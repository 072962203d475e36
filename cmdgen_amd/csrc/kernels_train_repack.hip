// kernels_train_repack.hip - the per-step re-packing of the parameters the optimizer has just updated: the fp32 fragment orders, the split
// fragment packs of the data gradients and the half-engine packs of the training forward (layouts: cmdgen_wlayout.h; the table structs:
// cmdgen_train_kernels.h).
#include "cmdgen_train_parts.h"

// ------------------------------------------------------------------------------------
// Per-step re-pack of the parameters the optimizer has just updated into the layouts the fused evaluation kernels
// stream (fragment orders: cmdgen_wlayout.h): every block's six Linears in both fp32 fragment orders, the transposed embedding
// tables and the radial / d0 weight columns.  Two table-driven launches; ~36 MB of traffic per step.
// ------------------------------------------------------------------------------------
// element [row][k] of the matrix a RepackFrag / RepackHalf16 entry packs (row_split / col_shift: cmdgen_train_kernels.h)
template <class F>
__device__ __forceinline__ const float* repack_src(const float* theta, const F& f, int row, int k) {
    int c = k, r = row;
    if (f.row_split && row >= f.row_split) { c = k + f.col_shift; r = row - f.row_split; }
    return theta + f.src_off + (size_t)r * f.ld + c;
}
template <class FR>     // the piece of thread idx = (nt * KB + kb) * 64 + lane = wfrag_piece(nt * KB + kb, 1, 0, lane) of one fp32 order
__device__ __forceinline__ float4 repack_frag_f32(const float* theta, const RepackFrag& f, int idx) {
    const int KB = f.in / FR::KBLK, lane = idx & 63, kb = (idx >> 6) % KB, nt = (idx >> 6) / KB;
    const float* src = repack_src(theta, f, FR::row(nt, lane), FR::k0(kb, lane));
    return make_float4(src[0], src[1], src[2], src[3]);
}
__global__ void k_repack_frags(const float* __restrict__ theta, const RepackFrag* __restrict__ tab) {
    const RepackFrag f = tab[blockIdx.y];
    const int n4 = f.out * f.in / 4;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n4) return;
    reinterpret_cast<float4*>(f.dst32)[idx] = repack_frag_f32<WFrag<32, 4>>(theta, f, idx);
    reinterpret_cast<float4*>(f.dst16)[idx] = repack_frag_f32<WFrag<16, 4>>(theta, f, idx);
}
__global__ void k_repack_misc(const float* __restrict__ theta, const RepackMisc* __restrict__ tab) {
    const RepackMisc m = tab[blockIdx.y];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m.rows * m.cols) return;
    const int c = idx / m.rows, r = idx - c * m.rows;
    m.dst[idx] = theta[m.src_off + (size_t)r * m.ld + c];
}
void tr_repack(const float* theta, const void* frag_tab, int n_frag, int max_frag4, const void* misc_tab, int n_misc, int max_misc,
               hipStream_t s) {
    hipLaunchKernelGGL(k_repack_frags, dim3((max_frag4 + 255) / 256, n_frag), dim3(256), 0, s, theta, (const RepackFrag*)frag_tab);
    hipLaunchKernelGGL(k_repack_misc, dim3((max_misc + 255) / 256, n_misc), dim3(256), 0, s, theta, (const RepackMisc*)misc_tab);
}
// split fragment packs (WPack::ws order, cmdgen_wlayout.h) of 256 x 256 weight sub-blocks or of their transposes (RepackSplitT)
__global__ void k_repack_split_t(const float* __restrict__ theta, const RepackSplitT* __restrict__ tab) {
    typedef WFrag<32, 8> FR;
    const RepackSplitT f = tab[blockIdx.y];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;         // (nt * 16 + kb) * 64 + lane, nt < 8, kb < 16
    if (idx >= 8 * 16 * 64) return;
    const int lane = idx & 63, kb = (idx >> 6) & 15, nt = idx >> 10;
    const int o = FR::row(nt, lane), k = FR::k0(kb, lane);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = f.transpose ? theta[f.src_off + (size_t)(k + j) * f.ld + o] : theta[f.src_off + (size_t)o * f.ld + k + j];
    sbf16x8 p0, p1, p2;
    split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), p0, p1, p2);
    sbf16x8* d = reinterpret_cast<sbf16x8*>(f.dst) + wfrag_piece(nt * 16 + kb, 3, 0, lane);
    d[0] = p0; d[64] = p1; d[128] = p2;
}
void tr_repack_split_t(const float* theta, const void* tab, int n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_repack_split_t, dim3(8 * 16 * 64 / 256, n), dim3(256), 0, s, theta, (const RepackSplitT*)tab);
}
// Half-engine packs of the training forward's two edge kernels (cmdgen_split.h, "half" engine), re-made every step like the split packs:
// two fp16 pieces of (w * 2^e) per weight (WPack::wh order and whalf_exp, cmdgen_wlayout.h), e chosen ON THE DEVICE - the parameters move
// every step, no host value can be trusted - and sc = {2^e, 2^-e} left beside the pack for the kernel's epilogue (WPack::wh_dev).  One
// workgroup of 1024 threads per 256 x 256 matrix: the 64 weights a thread packs stay in its registers between the maximum and the split.
template <bool TR>      // TR: the entries are transposed blocks (a strided gather; its own instantiation: sharing one cost the plain packs 20 us per step)
__global__ __launch_bounds__(1024) void k_repack_half(const float* __restrict__ theta, const RepackHalf* __restrict__ tab) {
    typedef WFrag<32, 8> FR;
    const RepackHalf f = tab[blockIdx.x];
    __shared__ float red[16];
    const int tid = threadIdx.x;
    float4 va[8], vb[8];
    float mx = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int idx = q * 1024 + tid;                                // (nt * 16 + kb) * 64 + lane, nt < 8, kb < 16
        const int lane = idx & 63, kb = (idx >> 6) & 15, nt = idx >> 10;
        const int o = FR::row(nt, lane), k = FR::k0(kb, lane);
        if constexpr (TR) {                                            // Wt[o][k] = W[k][o]
            const float* src = theta + f.src_off + (size_t)k * f.ld + o;
            va[q] = make_float4(src[0], src[(size_t)f.ld], src[2 * (size_t)f.ld], src[3 * (size_t)f.ld]);
            vb[q] = make_float4(src[4 * (size_t)f.ld], src[5 * (size_t)f.ld], src[6 * (size_t)f.ld], src[7 * (size_t)f.ld]);
        } else {
            const float4* src = reinterpret_cast<const float4*>(theta + f.src_off + (size_t)o * f.ld + k);
            va[q] = src[0]; vb[q] = src[1];
        }
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(va[q].x), fabsf(va[q].y)), fmaxf(fabsf(va[q].z), fabsf(va[q].w))));
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(vb[q].x), fabsf(vb[q].y)), fmaxf(fabsf(vb[q].z), fabsf(vb[q].w))));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, red[i]);
    const int e = whalf_exp(mx);
    const float sc = whalf_pow2(e);
    if (tid == 0) { f.sc[0] = sc; f.sc[1] = whalf_pow2(-e); }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int idx = q * 1024 + tid;
        const int lane = idx & 63;
        const float w[8] = {va[q].x * sc, va[q].y * sc, va[q].z * sc, va[q].w * sc, vb[q].x * sc, vb[q].y * sc, vb[q].z * sc, vb[q].w * sc};
        union { _Float16 h[8]; uint4 u; } p0, p1;
#pragma unroll
        for (int j = 0; j < 8; ++j) { p0.h[j] = (_Float16)w[j]; p1.h[j] = (_Float16)(w[j] - (float)p0.h[j]); }
        uint4* d = reinterpret_cast<uint4*>(f.dst) + wfrag_piece(idx >> 6, 2, 0, lane);
        d[0] = p0.u; d[64] = p1.u;
    }
}
// entries [0, n_plain) are packs of W itself, [n_plain, n) of transposed blocks (the table's order, cmdgen_train.hip)
void tr_repack_half(const float* theta, const void* tab, int n_plain, int n, hipStream_t s) {
    if (n_plain) hipLaunchKernelGGL(k_repack_half<false>, dim3(n_plain), dim3(1024), 0, s, theta, (const RepackHalf*)tab);
    if (n > n_plain) hipLaunchKernelGGL(k_repack_half<true>, dim3(n - n_plain), dim3(1024), 0, s, theta, (const RepackHalf*)tab + n_plain);
}
// The same for the node kernel of the training forward (k_node16w<true>): the 16-row half packs (WPack::wh16 order, cmdgen_wlayout.h) of
// node_mlp.0 [H][2H], node_mlp.2 [H][H] and the stacked projections [2H][H] of coord_mlp.0 / edge_mlp.0 (row_split / col_shift).  A pack
// has ONE scale (its products share accumulators), so the maximum is a launch of its own: k_wmax16 (one workgroup per pack) leaves
// {2^e, 2^-e}, k_repack_half16 splits.
__global__ __launch_bounds__(1024) void k_wmax16(const float* __restrict__ theta, const RepackHalf16* __restrict__ tab) {
    const RepackHalf16 f = tab[blockIdx.x];
    __shared__ float red[16];
    const int tid = threadIdx.x, n4 = f.out * f.in / 4, k4 = f.in / 4;
    float mx = 0.f;
    const int sh = 31 - __clz(k4);                                      // in is 256 or 512: k4 a power of two (no integer division per element)
#pragma unroll 4
    for (int i = tid; i < n4; i += 1024) {
        const float2* src = reinterpret_cast<const float2*>(repack_src(theta, f, i >> sh, 4 * (i & (k4 - 1))));      // (every tensor starts 16-byte aligned, rows are an even number of floats)
        const float2 a = src[0], b = src[1];
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(b.x), fabsf(b.y))));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) {
        mx = red[0];
        for (int i = 1; i < 16; ++i) mx = fmaxf(mx, red[i]);
        const int e = whalf_exp(mx);
        f.sc[0] = whalf_pow2(e); f.sc[1] = whalf_pow2(-e);
    }
}
__global__ void k_repack_half16(const float* __restrict__ theta, const RepackHalf16* __restrict__ tab) {
    const RepackHalf16 f = tab[blockIdx.y];
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;         // (nt * KB + kb) * 64 + lane, nt < out / 16, kb < in / 32
    if (idx >= f.out * f.in / 8) return;
    typedef WFrag<16, 8> FR;
    const int KB = f.in / FR::KBLK, lane = idx & 63, kb = (idx >> 6) % KB, nt = (idx >> 6) / KB;
    const float sc = f.sc[0];
    const float* lo = repack_src(theta, f, FR::row(nt, lane), FR::k0(kb, lane));
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = lo[FR::koff(j)] * sc;
    union { _Float16 h[8]; uint4 u; } p0, p1;
#pragma unroll
    for (int j = 0; j < 8; ++j) { p0.h[j] = (_Float16)w[j]; p1.h[j] = (_Float16)(w[j] - (float)p0.h[j]); }
    uint4* d = reinterpret_cast<uint4*>(f.dst) + wfrag_piece(idx >> 6, 2, 0, lane);
    d[0] = p0.u; d[64] = p1.u;
}
void tr_repack_half16(const float* theta, const void* tab, int n, int max8, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_wmax16, dim3(n), dim3(1024), 0, s, theta, (const RepackHalf16*)tab);
    hipLaunchKernelGGL(k_repack_half16, dim3((max8 + 255) / 256, n), dim3(256), 0, s, theta, (const RepackHalf16*)tab);
}
