// kernels_train_adjoint.hip - the small adjoints of the training step's backward pass: SiLU' and scaling passes, column sums (bias, radial / d0
// and head weight gradients), the per-sample projection, the start of the pass and what the input-gradient pass adds; each with its launcher.
#include "cmdgen_train_parts.h"

// g <- g * SiLU'(pre)
__global__ void k_silu_bwd(float* __restrict__ g, const float* __restrict__ pre, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] *= dsilu(pre[i]);
}
__global__ void k_silu_bwd4(float4* __restrict__ g, const float4* __restrict__ pre, size_t n4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 p = pre[i]; float4 v = g[i];
    v.x *= dsilu(p.x); v.y *= dsilu(p.y); v.z *= dsilu(p.z); v.w *= dsilu(p.w);
    g[i] = v;
}
// x[row][:] /= div[row]  (aggregation 'mean': the receiver's edge count)
__global__ void k_scale_rows(float* __restrict__ x, const float* __restrict__ div, int H, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] / div[i / H];
}
__global__ void k_scale(float* __restrict__ x, float d, size_t n) {      // x /= d (a true division, as the reference)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] /= d;
}
// out[c * ldo] += sum_e s[e] * X[e][c]   (s may be null = 1): bias gradients, radial / d0 column gradients, att and
// coordinate-head weight gradients.  One workgroup per 256-row chunk, one column per thread (coalesced rows).
__global__ void k_colsum(int E, int ncols, const float* __restrict__ X, int ldx, const float* __restrict__ s,
                         float* __restrict__ out, int ldo) {
    const int c = threadIdx.x;
    if (c >= ncols) return;
    const int e0 = blockIdx.x * 32, e1 = min(E, e0 + 32);
    float acc = 0.f;
    for (int e = e0; e < e1; ++e) acc += (s ? s[e] : 1.0f) * X[(size_t)e * ldx + c];
    atomicAdd(out + (size_t)c * ldo, acc);
}
// aligned fast path (ncols % 4 == 0, ldx % 4 == 0, 16-byte aligned X): 128 rows per workgroup, a thread owns four
// columns of every fourth row (16-byte loads, independent accumulators), the four row groups are combined in LDS, so a
// workgroup issues ncols atomics for 128 rows instead of ncols per 32 rows (the atomics all hit the same few lines).
__global__ __launch_bounds__(256) void k_colsum4(int E, int ncols, const float* __restrict__ X, int ldx,
                                                 const float* __restrict__ s, float* __restrict__ out, int ldo) {
    __shared__ float4 red[4][64];
    const int cg = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int e0 = blockIdx.x * 128, e1 = min(E, e0 + 128);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * cg < ncols) {
#pragma unroll 4
        for (int e = e0 + rg; e < e1; e += 4) {
            const float4 v = *reinterpret_cast<const float4*>(X + (size_t)e * ldx + 4 * cg);
            const float w = s ? s[e] : 1.0f;
            acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
        }
    }
    red[rg][cg] = acc;
    __syncthreads();
    if (rg == 0 && 4 * cg < ncols) {
        const float4 a = red[0][cg], b = red[1][cg], c = red[2][cg], d = red[3][cg];
        float* o = out + (size_t)(4 * cg) * ldo;
        atomicAdd(o, (a.x + b.x) + (c.x + d.x));
        atomicAdd(o + ldo, (a.y + b.y) + (c.y + d.y));
        atomicAdd(o + 2 * (size_t)ldo, (a.z + b.z) + (c.z + d.z));
        atomicAdd(o + 3 * (size_t)ldo, (a.w + b.w) + (c.w + d.w));
    }
}

// v[n] -= mean over the nodes of n's sample (one wave per sample; phar rows then pocket rows).  The projection is
// symmetric, so the same kernel is its own adjoint (applied to the incoming velocity gradient in backward).
__global__ __launch_bounds__(64) void k_center_per_sample(Layout lay, float* __restrict__ v /* [N][4] */) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b], pb = lay.phar_base[b], qb = lay.Nl + lay.pocket_base[b];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = lane; i < nl + np; i += 64) {
        const float* p = v + (size_t)(i < nl ? pb + i : qb + i - nl) * 4;
        sx += p[0]; sy += p[1]; sz += p[2];
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
    const float c = fmaxf((float)(nl + np), 1.0f);
    sx /= c; sy /= c; sz /= c;
    for (int i = lane; i < nl + np; i += 64) {
        float* p = v + (size_t)(i < nl ? pb + i : qb + i - nl) * 4;
        p[0] -= sx; p[1] -= sy; p[2] -= sz;
    }
}
// split d_eps [n_rows][3+F] into dvel [N][4] (rows row0..) and ddec [n_rows][F]
__global__ void k_eps_bwd(int n_rows, int F, int row0, const float* __restrict__ deps, float* __restrict__ dvel,
                          float* __restrict__ ddec) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows * (3 + F)) return;
    const int n = i / (3 + F), k = i - n * (3 + F);
    if (k < 3) dvel[(size_t)(row0 + n) * 4 + k] = deps[i]; else ddec[(size_t)n * F + k - 3] = deps[i];
}

// ------------------------------------------------------------------------------------
// input gradients (cmdgen_train_backward_inputs): what the parameter pass does not form
// ------------------------------------------------------------------------------------
// geometry adjoint of the d0 edge feature, d0 = |x_i - x_j|^2 of the INPUT positions X0 (egnn_new.py:194): dX[i] += 2 (x_i - x_j) dd0,
// dX[j] -= the same.  One thread per edge of a list (the message list and the coordinate list are launched one after the other).
__global__ void k_d0_adjoint(int E, const int* __restrict__ row, const int* __restrict__ col, const float4* __restrict__ X0,
                             const float* __restrict__ dd0, float* __restrict__ dX) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int i = row[e], j = col[e];
    if (i == j) return;
    const float4 a = X0[i], b = X0[j];
    const float g = 2.0f * dd0[e];
    const float gx = (a.x - b.x) * g, gy = (a.y - b.y) * g, gz = (a.z - b.z) * g;
    float* p = dX + (size_t)i * 4; atomicAdd(p, gx); atomicAdd(p + 1, gy); atomicAdd(p + 2, gz);
    float* q = dX + (size_t)j * 4; atomicAdd(q, -gx); atomicAdd(q + 1, -gy); atomicAdd(q + 2, -gz);
}
// the batch-global NaN guard reset vel to zeros (dynamics.py:129-131): no gradient flows through vel at all - neither the direct term nor
// the network's path through x_final - so the input pass starts from dL/dvel = 0 (the parameter pass keeps its seed: the trainer's norm guard)
__global__ void k_zero_if_flag(float* __restrict__ v, size_t n, const int* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && *flag) v[i] = 0.f;
}
// position columns of the input gradients: dL/dx_in = dL/dx_0 (through the network, dX) - dL/dvel (the direct term of vel = x_final - x,
// dvel0: after the projection's adjoint; zero where the batch-global NaN guard reset vel).  Rows < Nl -> d_xh_phar, the rest -> d_xh_pocket.
__global__ void k_input_x(int Nl, int N, int ldp, int ldq, const float* __restrict__ dX, const float* __restrict__ dvel0,
                          const int* __restrict__ nan_flag, float* __restrict__ dxp, float* __restrict__ dxq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * 3) return;
    const int n = i / 3, k = i - n * 3;
    const float direct = *nan_flag ? 0.f : dvel0[(size_t)n * 4 + k];
    const float v = dX[(size_t)n * 4 + k] - direct;
    if (n < Nl) { if (dxp) dxp[(size_t)n * ldp + k] = v; }
    else if (dxq) dxq[(size_t)(n - Nl) * ldq + k] = v;
}
// d_t[b] = sum over the nodes of sample b of the time column of dL/d[enc_out | t] (condition_time: h_time = t[mask], dynamics.py:96-98).
// One wave per sample, phar rows then pocket rows.
__global__ __launch_bounds__(64) void k_dt(Layout lay, const float* __restrict__ dhdyn, int dyn, float* __restrict__ dt) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b], pb = lay.phar_base[b], qb = lay.Nl + lay.pocket_base[b];
    float sum = 0.f;
    for (int i = lane; i < nl + np; i += 64) sum += dhdyn[(size_t)(i < nl ? pb + i : qb + i - nl) * dyn + dyn - 1];
    sum = wave_sum(sum);
    if (lane == 0) dt[b] = sum;
}
// ------------------------------------------------------------------------------------
// launch helpers (C++ linkage, used by cmdgen_train.hip)
// ------------------------------------------------------------------------------------
#define EW_GRID(n) dim3((unsigned)(((size_t)(n) + 255) / 256)), dim3(256)
#define ROW_GRID(E) dim3((unsigned)(((E) + 3) / 4)), dim3(256)        // one wave per row, 4 rows per workgroup

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
void tr_silu_bwd(float* g, const float* pre, size_t n, hipStream_t s) {
    if (!n) return;
    if (n % 4 == 0 && al16(g) && al16(pre)) hipLaunchKernelGGL(k_silu_bwd4, EW_GRID(n / 4), 0, s, (float4*)g, (const float4*)pre, n / 4);
    else hipLaunchKernelGGL(k_silu_bwd, EW_GRID(n), 0, s, g, pre, n);
}
void tr_scale(float* x, float d, size_t n, hipStream_t s) { if (n) hipLaunchKernelGGL(k_scale, EW_GRID(n), 0, s, x, d, n); }
void tr_scale_rows(float* x, const float* div, int H, size_t n, hipStream_t s) { if (n) hipLaunchKernelGGL(k_scale_rows, EW_GRID(n), 0, s, x, div, H, n); }
void tr_colsum(int E, int ncols, const float* X, int ldx, const float* sv, float* out, int ldo, hipStream_t s) {
    if (!E) return;
    if (ncols % 4 == 0 && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 && ncols <= 256)
        hipLaunchKernelGGL(k_colsum4, dim3((E + 127) / 128), dim3(256), 0, s, E, ncols, X, ldx, sv, out, ldo);
    else
        hipLaunchKernelGGL(k_colsum, dim3((E + 31) / 32), dim3(256), 0, s, E, ncols, X, ldx, sv, out, ldo);
}
void tr_center_per_sample(const Layout& lay, float* v, hipStream_t s) {
    hipLaunchKernelGGL(k_center_per_sample, dim3(lay.B), dim3(64), 0, s, lay, v);
}
void tr_eps_bwd(int n_rows, int F, int row0, const float* deps, float* dvel, float* ddec, hipStream_t s) {
    if (n_rows) hipLaunchKernelGGL(k_eps_bwd, EW_GRID((size_t)n_rows * (3 + F)), 0, s, n_rows, F, row0, deps, dvel, ddec);
}
// start of the conditional model's backward pass in one launch instead of three fills and k_eps_bwd: dX <- the velocity part of d_eps on the phar
// rows and zero elsewhere (pocket rows do not move), ddec <- its feature part, dhfin <- 0
__global__ void k_bwd_init(int Nl, int N, int P, int dyn, const float* __restrict__ deps, float* __restrict__ dX, float* __restrict__ ddec,
                           float* __restrict__ dhfin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N * 4) { const int n = i >> 2, k = i & 3; dX[i] = (n < Nl && k < 3) ? deps[(size_t)n * (3 + P) + k] : 0.f; }
    if (i < Nl * P) { const int n = i / P, k = i - n * P; ddec[i] = deps[(size_t)n * (3 + P) + 3 + k]; }
    if (i < N * dyn) dhfin[i] = 0.f;
}
void tr_bwd_init(int Nl, int N, int P, int dyn, const float* deps, float* dX, float* ddec, float* dhfin, hipStream_t s) {
    const size_t n = (size_t)N * (dyn > 4 ? dyn : 4) > (size_t)Nl * P ? (size_t)N * (dyn > 4 ? dyn : 4) : (size_t)Nl * P;
    if (n) hipLaunchKernelGGL(k_bwd_init, EW_GRID(n), 0, s, Nl, N, P, dyn, deps, dX, ddec, dhfin);
}
void tr_zero_if_flag(float* v, size_t n, const int* flag, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_zero_if_flag, EW_GRID(n), 0, s, v, n, flag);
}
void tr_d0_adjoint(int E, const int* row, const int* col, const float4* X0, const float* dd0, float* dX, hipStream_t s) {
    if (E) hipLaunchKernelGGL(k_d0_adjoint, EW_GRID(E), 0, s, E, row, col, X0, dd0, dX);
}
void tr_input_x(int Nl, int N, int ldp, int ldq, const float* dX, const float* dvel0, const int* nan_flag, float* dxp, float* dxq, hipStream_t s) {
    if (N) hipLaunchKernelGGL(k_input_x, EW_GRID((size_t)N * 3), 0, s, Nl, N, ldp, ldq, dX, dvel0, nan_flag, dxp, dxq);
}
void tr_dt(const Layout& lay, const float* dhdyn, int dyn, float* dt, hipStream_t s) {
    if (lay.B) hipLaunchKernelGGL(k_dt, dim3(lay.B), dim3(64), 0, s, lay, dhdyn, dyn, dt);
}
