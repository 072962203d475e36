// kernels_train_gemm.hip - the GEMM kernels of the training step's backward pass: the generic training GEMM (exact fp32, or bf16 operands) of
// the fp32-instruction mode and of the small encoder / decoder products, and the grouped weight gradients (k_wgrad_group; k_wgrad_split and
// k_wgrad_split128 on the split-bf16 engine), each with its launcher.  Which kernel, grid and split-K a launch takes: cmdgen_train_plan.h.
// The training GEMM's staging and body are below; the weight gradients' staging and MFMA-order parts: cmdgen_train_parts.h.
#include "cmdgen_train_parts.h"
#include <type_traits>
#include <utility>

// ------------------------------------------------------------------------------------
// C[M,N] (+)= alpha * op(A)[M,K] * op(B)[K,N] (+ bias[N])          exact fp32 on v_mfma_f32_32x32x2_f32
//   TA = false: A stored [M][K] (lda)      TA = true: A stored [K][M] (lda)     (wgrad: A = dY^T)
//   TB = true : B stored [N][K] (ldb) - the nn.Linear weight layout (forward)
//   TB = false: B stored [K][N] (ldb) - dgrad (dX = dY W) and wgrad (dW = dY^T X)
// 64x64 tile per workgroup (4 waves, 32x32 each), K tile 16, both operands staged through LDS as
// [row][k] so that one ds_read_b128 per lane feeds four MFMA k-steps (same pairing as the sampler's
// tiles).  blockIdx.z splits K (wgrad over tens of thousands of edges); split results are combined with
// float atomics.  All loads are bounds-checked scalars: operands are arbitrary sub-blocks (column slices of
// edge_mlp.0, feature columns of xh) with arbitrary leading dimensions.
// k_sgemm_bf16: the same GEMM with bf16 OPERANDS and fp32 accumulation (v_mfma_f32_32x32x16_bf16: 16x the fp32 matrix rate) - the
// opt-in mixed-precision policy of the training step (master weights, optimizer state, activations in HBM and all
// elementwise math stay fp32).  One body, sgemm_tile; the two entry points keep the names the launch traces know.
// ------------------------------------------------------------------------------------
// k extent KT of one staged tile is a template parameter: 64 for launches with few workgroups (node-level products: one
// workgroup per CU, so fewer, fatter barrier-separated iterations and the register prefetch below are what hides the
// global latency), 32 for big launches (edge-level products: 18 KB of LDS per workgroup keeps 8 of them on a CU, which
// hides it better - 61 vs 54 TF/s on [25600,256]x[256,256]).
#define TG_LD(KT) ((KT) + 4)
#define TG_P(KT) ((KT) / 16)     // float4 fetches per thread and operand tile: 64 rows x KT k over 256 threads
#define TGH_LD(KT) ((KT) + 8)    // halfs per LDS row of the bf16 image: keeps the 16-byte operand reads aligned
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// One 64 x KT operand tile: fetch() brings this thread's TG_P float4 pieces into registers (so the NEXT tile's
// global loads are in flight while the current tile's MFMAs run - a small GEMM such as a node-level [3.8k,256]x[256,256]
// product has one workgroup per CU and nothing else to hide that latency behind), put_*() writes them to LDS as [row][k].
//   operand stored [row][k] (k contiguous): thread -> (row = tid/16 + 16*p, k4 = (tid%16)*4)
//   operand stored [k][row] (row contiguous): thread -> (k = tid/16 + 16*p, row4 = (tid%16)*4)
// VEC: every 4-element group a thread loads is 16-byte aligned and entirely in range (host-checked: base pointers,
// leading dimensions, the contiguous extent and the k chunking are multiples of 4) -> one global_load_dwordx4.
template <int KT, bool TRANS, bool VEC>
__device__ __forceinline__ void tg_fetch(float4 (&v)[TG_P(KT)], const float* __restrict__ G, int ld, int r0, int R, int k0, int k_end) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int p = 0; p < TG_P(KT); ++p) {
        v[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!TRANS) {
            constexpr int TPR = KT / 4, RPP = 256 / TPR;      // threads per row, rows per pass
            const int gr = r0 + tid / TPR + RPP * p, gk = k0 + (tid % TPR) * 4;
            if (gr < R) {
                const float* src = G + (size_t)gr * ld + gk;
                if (VEC && gk + 3 < k_end) v[p] = *reinterpret_cast<const float4*>(src);
                else {
                    if (gk < k_end) v[p].x = src[0];
                    if (gk + 1 < k_end) v[p].y = src[1];
                    if (gk + 2 < k_end) v[p].z = src[2];
                    if (gk + 3 < k_end) v[p].w = src[3];
                }
            }
        } else {
            const int gk = k0 + (tid >> 4) + 16 * p, gr = r0 + (tid & 15) * 4;
            if (gk < k_end) {
                const float* src = G + (size_t)gk * ld + gr;
                if (VEC && gr + 3 < R) v[p] = *reinterpret_cast<const float4*>(src);
                else {
                    if (gr < R) v[p].x = src[0];
                    if (gr + 1 < R) v[p].y = src[1];
                    if (gr + 2 < R) v[p].z = src[2];
                    if (gr + 3 < R) v[p].w = src[3];
                }
            }
        }
    }
}
template <int KT, bool TRANS>
__device__ __forceinline__ void tg_put_f32(float* S, const float4 (&v)[TG_P(KT)]) {
    const int tid = threadIdx.x;
    constexpr int TPR = KT / 4, RPP = 256 / TPR;
#pragma unroll
    for (int p = 0; p < TG_P(KT); ++p) {
        if (!TRANS) *reinterpret_cast<float4*>(S + (tid / TPR + RPP * p) * TG_LD(KT) + (tid % TPR) * 4) = v[p];
        else {
            const int k = (tid >> 4) + 16 * p, rq = (tid & 15) * 4;
            S[(rq + 0) * TG_LD(KT) + k] = v[p].x; S[(rq + 1) * TG_LD(KT) + k] = v[p].y;
            S[(rq + 2) * TG_LD(KT) + k] = v[p].z; S[(rq + 3) * TG_LD(KT) + k] = v[p].w;
        }
    }
}
__device__ __forceinline__ unsigned short f2bf(float f) {
    unsigned int u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);     // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
template <int KT, bool TRANS>
__device__ __forceinline__ void tg_put_bf16(unsigned short* S, const float4 (&v)[TG_P(KT)]) {
    const int tid = threadIdx.x;
    constexpr int TPR = KT / 4, RPP = 256 / TPR;
#pragma unroll
    for (int p = 0; p < TG_P(KT); ++p) {
        if (!TRANS) {
            uint2 pk;
            pk.x = (unsigned)f2bf(v[p].x) | ((unsigned)f2bf(v[p].y) << 16);
            pk.y = (unsigned)f2bf(v[p].z) | ((unsigned)f2bf(v[p].w) << 16);
            *reinterpret_cast<uint2*>(S + (tid / TPR + RPP * p) * TGH_LD(KT) + (tid % TPR) * 4) = pk;
        } else {
            const int k = (tid >> 4) + 16 * p, rq = (tid & 15) * 4;
            S[(rq + 0) * TGH_LD(KT) + k] = f2bf(v[p].x); S[(rq + 1) * TGH_LD(KT) + k] = f2bf(v[p].y);
            S[(rq + 2) * TGH_LD(KT) + k] = f2bf(v[p].z); S[(rq + 3) * TGH_LD(KT) + k] = f2bf(v[p].w);
        }
    }
}
// the MFMAs of one staged k tile, operands [row][k] in LDS.  fp32: one ds_read_b128 per lane feeds four v_mfma_f32_32x32x2_f32 k-steps;
// bf16: lanes 0-31 supply k 0..7, lanes 32-63 k 8..15 of a 16-k step of v_mfma_f32_32x32x16_bf16
template <int KT>
__device__ __forceinline__ void tg_ksteps_f32(f32x16& acc, const float* As, const float* Bs, int wm, int wn, int lane) {
#pragma unroll
    for (int kb = 0; kb < KT / 8; ++kb) {
        const float4 a = *reinterpret_cast<const float4*>(As + (wm + (lane & 31)) * TG_LD(KT) + kb * 8 + 4 * (lane >> 5));
        const float4 b = *reinterpret_cast<const float4*>(Bs + (wn + (lane & 31)) * TG_LD(KT) + kb * 8 + 4 * (lane >> 5));
        CMDGEN_MFMA32(acc, a.x, b.x);
        CMDGEN_MFMA32(acc, a.y, b.y);
        CMDGEN_MFMA32(acc, a.z, b.z);
        CMDGEN_MFMA32(acc, a.w, b.w);
    }
}
template <int KT>
__device__ __forceinline__ void tg_ksteps_bf16(f32x16& acc, const unsigned short* As, const unsigned short* Bs, int wm, int wn, int lane) {
#pragma unroll
    for (int ks = 0; ks < KT / 16; ++ks) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(As + (wm + (lane & 31)) * TGH_LD(KT) + ks * 16 + 8 * (lane >> 5));
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + (wn + (lane & 31)) * TGH_LD(KT) + ks * 16 + 8 * (lane >> 5));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
}

// shared epilogue: C (+)= alpha * acc + bias, split-K partials by atomics, the two SiLU epilogues
__device__ __forceinline__ void tg_epilogue(const f32x16& acc, int M, int N, float* __restrict__ C, int ldc,
                                            const float* __restrict__ bias, float alpha, int accumulate, int epi,
                                            float* __restrict__ aux, int ldaux) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int gn = n0 + wn + (lane & 31);
    if (gn >= N) return;
    const float bv = (bias && blockIdx.z == 0) ? bias[gn] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (gm >= M) continue;
        float* c = C + (size_t)gm * ldc + gn;
        float v = alpha * acc[r] + bv;
        if (gridDim.z > 1) { atomicAdd(c, v); continue; }
        if (accumulate) v += *c;
        // epilogues (never with split-K): 1 = also write SiLU(v) to aux (forward: pre-activation and activation in one
        // pass); 2 = multiply by SiLU'(aux) (dgrad through the activation that produced this operand)
        if (epi == 2) v *= dsilu(aux[(size_t)gm * ldaux + gn]);
        *c = v;
        if (epi == 1) aux[(size_t)gm * ldaux + gn] = silu_exact(v);
    }
}

// C[M,N] (+)= alpha * op(A)[M,K] * op(B)[K,N] (+ bias[N]): the body of k_sgemm (BF = false: exact fp32) and k_sgemm_bf16 (operands rounded
// to nearest-even bf16 while they are staged into LDS, fp32 accumulation).  The two differ in the LDS image, the put and the k-steps.
template <bool BF, int KT, bool TA, bool TB, bool VECA, bool VECB>
__device__ __forceinline__ void sgemm_tile(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                                           float* C, int ldc, const float* bias, float alpha, int accumulate,
                                           int kchunk, int epi, float* aux, int ldaux) {
    typedef typename std::conditional<BF, unsigned short, float>::type T;
    constexpr int LD = BF ? TGH_LD(KT) : TG_LD(KT);
    __shared__ __attribute__((aligned(16))) T As[64 * LD];
    __shared__ __attribute__((aligned(16))) T Bs[64 * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int k_begin = blockIdx.z * kchunk, k_end = min(K, k_begin + kchunk);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float4 ra[TG_P(KT)], rb[TG_P(KT)];
    tg_fetch<KT, TA, VECA>(ra, A, lda, m0, M, k_begin, k_end);
    tg_fetch<KT, !TB, VECB>(rb, B, ldb, n0, N, k_begin, k_end);
    for (int k0 = k_begin; k0 < k_end; k0 += KT) {
        if constexpr (BF) { tg_put_bf16<KT, TA>(As, ra); tg_put_bf16<KT, !TB>(Bs, rb); }
        else { tg_put_f32<KT, TA>(As, ra); tg_put_f32<KT, !TB>(Bs, rb); }
        __syncthreads();
        if (k0 + KT < k_end) {                        // next tile's loads fly during this tile's MFMAs
            tg_fetch<KT, TA, VECA>(ra, A, lda, m0, M, k0 + KT, k_end);
            tg_fetch<KT, !TB, VECB>(rb, B, ldb, n0, N, k0 + KT, k_end);
        }
        if constexpr (BF) tg_ksteps_bf16<KT>(acc, As, Bs, wm, wn, lane);
        else tg_ksteps_f32<KT>(acc, As, Bs, wm, wn, lane);
        __syncthreads();
    }
    tg_epilogue(acc, M, N, C, ldc, bias, alpha, accumulate, epi, aux, ldaux);
}

#define SGEMM_PARAMS int M, int N, int K, const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, float* __restrict__ C, int ldc, \
                     const float* __restrict__ bias, float alpha, int accumulate, int kchunk, int epi, float* __restrict__ aux, int ldaux
#define SGEMM_ARGS M, N, K, A, lda, B, ldb, C, ldc, bias, alpha, accumulate, kchunk, epi, aux, ldaux
template <int KT, bool TA, bool TB, bool VECA, bool VECB>
__global__ __launch_bounds__(256) void k_sgemm(SGEMM_PARAMS) { sgemm_tile<false, KT, TA, TB, VECA, VECB>(SGEMM_ARGS); }
template <int KT, bool TA, bool TB, bool VECA, bool VECB>
__global__ __launch_bounds__(256) void k_sgemm_bf16(SGEMM_PARAMS) { sgemm_tile<true, KT, TA, TB, VECA, VECB>(SGEMM_ARGS); }

// ------------------------------------------------------------------------------------
// Grouped weight gradients: up to 8 products dW_p (+)= dY_p^T X_p (and, optionally, db_p += column sums of dY_p) in ONE
// launch.  The node-level weight gradients of a block are seven [256 x 256] products over K = #nodes: each alone is a
// 16-tile launch that needs split-K to fill the chip and still costs ~23 us of launch + atomic latency; together they
// are one launch of the same duration.  Operands: dY_p [K][M_p] (lddy), X_p [K][N_p] (ldx), both 16-byte aligned with
// leading dimensions that are multiples of 4; results are added with float atomics (the destination holds the running
// gradient).  blockIdx.z = problem * zsplit + k-split.
// ------------------------------------------------------------------------------------
template <bool BF, bool XS = false>      // XS: some X_p holds pre-activations (WgradBatch::xs) - a separate instantiation: the default one carries no trace of it
__global__ __launch_bounds__(256) void k_wgrad_group(WgradBatch g, int K, int kchunk, int zsplit) {
    constexpr int KT = 64;
    // fp32 path: both operands lie in memory k-major ([k][channel]) and stay that way in LDS ([k][WG_LDK]): v_mfma_f32_32x32x2
    // takes ONE value per lane (row = lane % 32, k = lane / 32), so a wave reads 32 consecutive channels of two k rows per
    // MFMA straight from the staged rows - no transposition on the way in (the [channel][k] image needed scalar, bank-
    // conflicting LDS stores: 32 per thread and k step).  WG_LDK = 96: the two k rows of a read fall on disjoint banks.
    constexpr int WG_LDK = 96;
    __shared__ __attribute__((aligned(16))) float smem[2 * KT * WG_LDK];
    float* As = smem; float* Bs = smem + KT * WG_LDK;
    unsigned short* Ah = reinterpret_cast<unsigned short*>(smem);
    unsigned short* Bh = Ah + 64 * TGH_LD(KT);
    const int p = blockIdx.z / zsplit, kz = blockIdx.z - p * zsplit;
    const int M = g.M[p], N = g.N[p];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    if (m0 >= M || n0 >= N) return;
    const int k_begin = kz * kchunk, k_end = min(K, k_begin + kchunk);
    if (k_begin >= k_end) return;
    const float* __restrict__ A = g.dy[p]; const float* __restrict__ B = g.x[p];
    const int lda = g.lddy[p], ldb = g.ldx[p];
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const bool want_bias = g.db[p] != nullptr && n0 == 0;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float4 ra[TG_P(KT)], rb[TG_P(KT)];
    float4 colsum = make_float4(0.f, 0.f, 0.f, 0.f);      // this thread's rows m0 + (tid&15)*4 .. +3, its k slots
    tg_fetch<KT, true, true>(ra, A, lda, m0, M, k_begin, k_end);
    tg_fetch<KT, true, true>(rb, B, ldb, n0, N, k_begin, k_end);
    for (int k0 = k_begin; k0 < k_end; k0 += KT) {
        if (want_bias) {
#pragma unroll
            for (int q = 0; q < TG_P(KT); ++q) { colsum.x += ra[q].x; colsum.y += ra[q].y; colsum.z += ra[q].z; colsum.w += ra[q].w; }
        }
        if constexpr (XS) if (g.xs[p]) {
#pragma unroll
            for (int q = 0; q < TG_P(KT); ++q) rb[q] = silu4(rb[q]);
        }
        if (BF) { tg_put_bf16<KT, true>(Ah, ra); tg_put_bf16<KT, true>(Bh, rb); }
        else {
#pragma unroll
            for (int q = 0; q < TG_P(KT); ++q) {        // thread -> (k = tid / 16 + 16 q, channels (tid % 16) * 4 .. + 3), as fetched
                *reinterpret_cast<float4*>(As + ((tid >> 4) + 16 * q) * WG_LDK + (tid & 15) * 4) = ra[q];
                *reinterpret_cast<float4*>(Bs + ((tid >> 4) + 16 * q) * WG_LDK + (tid & 15) * 4) = rb[q];
            }
        }
        __syncthreads();
        if (k0 + KT < k_end) {
            tg_fetch<KT, true, true>(ra, A, lda, m0, M, k0 + KT, k_end);
            tg_fetch<KT, true, true>(rb, B, ldb, n0, N, k0 + KT, k_end);
        }
        if (BF) tg_ksteps_bf16<KT>(acc, Ah, Bh, wm, wn, lane);
        else {
            const float* ap = As + (lane >> 5) * WG_LDK + wm + (lane & 31);
            const float* bp = Bs + (lane >> 5) * WG_LDK + wn + (lane & 31);
#pragma unroll
            for (int k2 = 0; k2 < KT / 2; ++k2) CMDGEN_MFMA32(acc, ap[k2 * 2 * WG_LDK], bp[k2 * 2 * WG_LDK]);
        }
        __syncthreads();
    }
    float* C = g.dw[p];
    const int ldc = g.ldw[p];
    const int gn = n0 + wn + (lane & 31);
    if (gn < N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int gm = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (gm < M) atomicAdd(C + (size_t)gm * ldc + gn, acc[r]);
        }
    }
    if (want_bias) {            // 16 threads (tid >> 4) hold partial sums of the same four rows: combine through LDS
        float* red = smem;       // [16][64]
        const int rq = (tid & 15) * 4, slot = tid >> 4;
        red[slot * 64 + rq + 0] = colsum.x; red[slot * 64 + rq + 1] = colsum.y;
        red[slot * 64 + rq + 2] = colsum.z; red[slot * 64 + rq + 3] = colsum.w;
        __syncthreads();
        if (tid < 64 && m0 + tid < M) {
            float sum = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) sum += red[q * 64 + tid];
            atomicAdd(g.db[p] + m0 + tid, sum);
        }
    }
}

// ------------------------------------------------------------------------------------
// The same grouped products on the split-bf16 engine (cmdgen_split.h; every M_p, N_p a multiple of 64, operands 16-byte
// aligned): the fp32 instruction needs 512 matrix-pipe cycles per 16 k values of a 32 x 32 tile, six bf16 MFMAs need 192.
// BOTH operands are activations here, so both are split while they are staged: a thread loads eight consecutive k rows of
// four channels (8 x 16 bytes), splits the eight k values of each channel into the three bf16 pieces in registers (the
// fragment layout of v_mfma_f32_32x32x16_bf16 wants eight consecutive k per lane: the k-major memory layout is transposed
// in registers, not with scalar LDS stores) and writes one 16-byte piece per channel and plane: planes [channel][64 + 8].
// Threads 0-127 stage dY, 128-255 stage X; the next k tile's rows are in flight during the MFMAs.  NPC = 1: leading pieces
// only (bf16 operands).
// ------------------------------------------------------------------------------------
template <int NPC, bool XS = false>
__global__ __launch_bounds__(256, 2) void k_wgrad_split(WgradBatch g, int K, int kchunk, int zsplit) {
    constexpr int KT = 64, PLD = KT + 8, PE = 64 * PLD;               // bf16 elements per plane row / per plane
    __shared__ __attribute__((aligned(16))) unsigned short planes[2 * NPC * PE];
    const int p = blockIdx.z / zsplit, kz = blockIdx.z - p * zsplit;
    const int M = g.M[p], N = g.N[p];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    if (m0 >= M || n0 >= N) return;
    const int k_begin = kz * kchunk, k_end = min(K, k_begin + kchunk);
    if (k_begin >= k_end) return;
    const bool isB = tid >= 128;
    const int t = tid & 127, cg = t & 15, kb = t >> 4;                 // channels 4 cg .. 4 cg + 3, k rows 8 kb .. 8 kb + 7 of the tile
    const float* __restrict__ G = isB ? g.x[p] : g.dy[p];
    const int ld = isB ? g.ldx[p] : g.lddy[p];
    const float* gsrc = G + (isB ? n0 : m0) + 4 * cg;
    unsigned short* mine = planes + (isB ? NPC * PE : 0);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const bool want_bias = g.db[p] != nullptr && n0 == 0 && !isB;
    f32x16 acc[1][1];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[0][0][i] = 0.f;
    float4 v[8];
    float4 colsum = make_float4(0.f, 0.f, 0.f, 0.f);
    wg_fetch8(v, gsrc, ld, k_begin + 8 * kb, k_end);
    for (int k0 = k_begin; k0 < k_end; k0 += KT) {
        if (want_bias) wg_colsum8(colsum, v);
        if constexpr (XS) if (isB && g.xs[p]) wg_silu8(v);
        wg_stage8<NPC>(v, PE, [&](int c) { return mine + (4 * cg + c) * PLD + 8 * kb; });
        __syncthreads();
        if (k0 + KT < k_end) wg_fetch8(v, gsrc, ld, k0 + KT + 8 * kb, k_end);
        const unsigned short* ap = planes + (wm + (lane & 31)) * PLD + 8 * (lane >> 5);
        const unsigned short* bp = planes + NPC * PE + (wn + (lane & 31)) * PLD + 8 * (lane >> 5);
#pragma unroll
        for (int ks = 0; ks < KT / 16; ++ks) {
            sbf16x8 a[1][NPC], b[1][NPC];
#pragma unroll
            for (int q = 0; q < NPC; ++q) {
                a[0][q] = *reinterpret_cast<const sbf16x8*>(ap + q * PE + ks * 16);
                b[0][q] = *reinterpret_cast<const sbf16x8*>(bp + q * PE + ks * 16);
            }
            split_mfmas<NPC>(acc, a, b);
        }
        __syncthreads();
    }
    float* C = g.dw[p];
    const int ldc = g.ldw[p];
    const int gn = n0 + wn + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        atomicAdd(C + (size_t)gm * ldc + gn, acc[0][0][r]);
    }
    if (g.db[p] != nullptr && n0 == 0) {   // 8 threads (kb) hold partial sums of the same four channels: combine through LDS
        float* red = reinterpret_cast<float*>(planes);       // [8][64]
        if (!isB) *reinterpret_cast<float4*>(red + kb * 64 + 4 * cg) = colsum;
        __syncthreads();
        if (tid < 64) {
            float sum = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) sum += red[q * 64 + tid];
            atomicAdd(g.db[p] + m0 + tid, sum);
        }
    }
}

// ------------------------------------------------------------------------------------
// k_wgrad_split128: the same products on 128 x 128 output tiles (round 3).  k_wgrad_split's 64 x 64 tile gives a wave ONE
// 32 x 32 accumulator: six 16-byte LDS reads per six MFMAs (144 KB of LDS reads per 64 k values of a tile - the LDS pipe, not the
// matrix pipe, bound it, and three-piece weight gradients only tied the fp32 instruction).  Here a wave owns 64 x 64 (2 x 2
// accumulators): twelve reads per 24 MFMAs, half the LDS bytes per FLOP; k tiles of 32 keep the two operands' planes at 60 KB
// (two workgroups per CU: one stages and splits while the other multiplies).  Staging as before - a thread transposes eight
// consecutive k rows of four channels in registers and writes one 16-byte piece per channel and plane - with the k-octet
// position XOR-swizzled by the channel group, so the sixteen lanes of a store cycle fall on sixteen different bank groups
// (channel rows four apart put them on four).  Every M_p, N_p a multiple of 128.
// ------------------------------------------------------------------------------------
template <int NPC, bool XS = false>
__global__ __launch_bounds__(256, 2) void k_wgrad_split128(WgradBatch g, int K, int kchunk, int zsplit) {
    constexpr int KT = 32, PLD = KT + 8, TM = 128, PE = TM * PLD;     // bf16 elements per plane row / per plane
    __shared__ __attribute__((aligned(16))) unsigned short planes[2 * NPC * PE];
    const int p = blockIdx.z / zsplit, kz = blockIdx.z - p * zsplit;
    const int M = g.M[p], N = g.N[p];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TM;
    if (m0 >= M || n0 >= N) return;
    const int k_begin = kz * kchunk, k_end = min(K, k_begin + kchunk);
    if (k_begin >= k_end) return;
    const bool isB = tid >= 128;
    const int t = tid & 127, cg = t & 31, kb = t >> 5;                 // channels 4 cg .. 4 cg + 3, k rows 8 kb .. 8 kb + 7 of the tile
    const float* __restrict__ G = isB ? g.x[p] : g.dy[p];
    const int ld = isB ? g.ldx[p] : g.lddy[p];
    const float* gsrc = G + (isB ? n0 : m0) + 4 * cg;
    // octet kb of channel row ch lies at element 8 (kb ^ ((ch >> 4) & 3)) of the row
    unsigned short* mine = planes + (isB ? NPC * PE : 0) + 4 * cg * PLD + 8 * (kb ^ ((cg >> 2) & 3));
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const bool want_bias = g.db[p] != nullptr && n0 == 0 && !isB;
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.f;
    float4 v[8];
    float4 colsum = make_float4(0.f, 0.f, 0.f, 0.f);
    // fragment rows of this lane: row (lane & 31) of each 32-row tile, k octet (lane >> 5) of a 16-k block; (row >> 4) & 3 = 2 (tile & 1) + ((lane >> 4) & 1)
    const int lrow = lane & 31, loct = lane >> 5, lsw = (lane >> 4) & 1;
    wg_fetch8(v, gsrc, ld, k_begin + 8 * kb, k_end);
    for (int k0 = k_begin; k0 < k_end; k0 += KT) {
        if (want_bias) wg_colsum8(colsum, v);
        if constexpr (XS) if (isB && g.xs[p]) wg_silu8(v);
        wg_stage8<NPC>(v, PE, [&](int c) { return mine + c * PLD; });
        __syncthreads();
        if (k0 + KT < k_end) wg_fetch8(v, gsrc, ld, k0 + KT + 8 * kb, k_end);
#pragma unroll
        for (int ks = 0; ks < KT / 16; ++ks) {
            sbf16x8 a[2][NPC], b[2][NPC];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                // tile rows wm + 32 m + lrow (wm a multiple of 64): channel group bits (row >> 4) & 3 = 2 m + lsw
                const int oa = (wm + 32 * m + lrow) * PLD + 8 * ((2 * ks + loct) ^ (2 * m + lsw));
                const int ob = NPC * PE + (wn + 32 * m + lrow) * PLD + 8 * ((2 * ks + loct) ^ (2 * m + lsw));
#pragma unroll
                for (int q = 0; q < NPC; ++q) {
                    a[m][q] = *reinterpret_cast<const sbf16x8*>(planes + oa + q * PE);
                    b[m][q] = *reinterpret_cast<const sbf16x8*>(planes + ob + q * PE);
                }
            }
            split_mfmas<NPC>(acc, a, b);
        }
        __syncthreads();
    }
    float* C = g.dw[p];
    const int ldc = g.ldw[p];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int gn = n0 + wn + 32 * n + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gm = m0 + wm + 32 * m + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                atomicAdd(C + (size_t)gm * ldc + gn, acc[m][n][r]);
            }
        }
    if (g.db[p] != nullptr && n0 == 0) {   // 4 threads (kb) hold partial sums of the same four channels: combine through LDS
        float* red = reinterpret_cast<float*>(planes);       // [4][128]
        if (!isB) *reinterpret_cast<float4*>(red + kb * TM + 4 * cg) = colsum;
        __syncthreads();
        if (tid < TM) atomicAdd(g.db[p] + m0 + tid, (red[tid] + red[TM + tid]) + (red[2 * TM + tid] + red[3 * TM + tid]));
    }
}

// the kernel, grid and split-K of a group: plan_wgrad (cmdgen_train_plan.h); here only what needs a pointer - the alignment test and the launch
void cmdgen_wgrad_group(const WgradBatch& g, int K, bool bf16, hipStream_t s, const TrainTune& tune, bool split3, bool force3) {
    if (g.n <= 0 || K <= 0) return;
    WgradShapes sh; sh.n = g.n;
    for (int p = 0; p < g.n; ++p)
        sh.p[p] = WgradShape{g.M[p], g.N[p], g.lddy[p] % 4, g.ldx[p] % 4,
                             (reinterpret_cast<uintptr_t>(g.dy[p]) & 15) == 0 && (reinterpret_cast<uintptr_t>(g.x[p]) & 15) == 0, g.xs[p]};
    const WgradPlan pl = plan_wgrad(sh, K, bf16, split3, force3, tune);
    typedef void (*Kernel)(WgradBatch, int, int, int);
    static const Kernel tab[3][2][2] = {       // [WgradKernel][bf16 operands][xs]
        {{k_wgrad_group<false>, k_wgrad_group<false, true>}, {k_wgrad_group<true>, k_wgrad_group<true, true>}},
        {{k_wgrad_split<3>, k_wgrad_split<3, true>}, {k_wgrad_split<1>, k_wgrad_split<1, true>}},
        {{k_wgrad_split128<3>, k_wgrad_split128<3, true>}, {k_wgrad_split128<1>, k_wgrad_split128<1, true>}}};
    hipLaunchKernelGGL(tab[(int)pl.kernel][pl.pieces == 1][pl.xs], dim3(pl.grid[0], pl.grid[1], pl.grid[2]), dim3(256), 0, s, g, K, pl.kchunk, pl.zsplit);
}
// the 64 instantiations of the training GEMM, indexed by SgemmPlan::slot(): bf16 operands, the 64-wide k tile, ta, tb, VECA, VECB
typedef void (*SgemmKernel)(int, int, int, const float*, int, const float*, int, float*, int, const float*, float, int, int, int, float*, int);
template <int I> static SgemmKernel sgemm_kernel() {
    constexpr int KT = (I & 16) ? 64 : 32;
    constexpr bool TA = (I & 8) != 0, TB = (I & 4) != 0, VA = (I & 2) != 0, VB = (I & 1) != 0;
    if constexpr ((I & 32) != 0) return k_sgemm_bf16<KT, TA, TB, VA, VB>; else return k_sgemm<KT, TA, TB, VA, VB>;
}
template <int... I> static SgemmKernel sgemm_kernel_of(int slot, std::integer_sequence<int, I...>) {
    static const SgemmKernel tab[] = {sgemm_kernel<I>()...};
    return tab[slot];
}
void cmdgen_sgemm(bool ta, bool tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                  int ldc, const float* bias, float alpha, bool accumulate, int split_k, hipStream_t s,
                  int epi, float* aux, int ldaux, bool bf16) {
    if (M <= 0 || N <= 0 || K <= 0) return;
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    // weights inside the flat buffer may be unaligned
    const SgemmPlan pl = plan_sgemm(ta, tb, M, N, K, al(A) && (lda % 4 == 0), al(B) && (ldb % 4 == 0), split_k, bf16, epi);
    // split-K partials are combined with atomics: the destination must already hold the value to add to
    hipLaunchKernelGGL(sgemm_kernel_of(pl.slot(), std::make_integer_sequence<int, 64>{}), dim3(pl.grid[0], pl.grid[1], pl.grid[2]), dim3(256), 0, s,
                       M, N, K, A, lda, B, ldb, C, ldc, bias, alpha, accumulate ? 1 : 0, pl.kchunk, pl.epi, aux, ldaux);
}
