// kernels_inpaint.hip - RePaint for the CONDITIONAL model (ConditionalDDPM.inpaint, cmdgen_inpaint_chain): the ancestral
// sampler of kernels_ddpm.hip with some phar rows held at a noised copy of known input rows.  One op of the schedule
// (get_repaint_schedule, en_diffusion.py:649-670), going from t to s, is
//   A  (z_u, P_u) = sample_p_zs_given_zt(s, t, z, P)                       (conditional_model.py:342-374)
//   B  z_k = alpha_s K + sigma_s eps_B, then z_k.x += com(P_u) - com(P0)  (the noised known rows in the current frame)
//      z.x = fix_x ? z_k.x : z_u.x, z.h = fix_h ? z_k.h : z_u.h, then remove_mean_batch(z.x, P_u.x)
//                                                                         (skipped for a sample without a mark)
//   C  if the schedule jumps back: (z, P) = sample_p_zt_given_zs(z, P, gamma(s + jump), gamma(s))   (:330-340)
// with K the normalised known rows and P0 the normalised input pocket.  z_T and the final decode are k_chain_init and
// k_chain_final of kernels_ddpm.hip.  com(P) - com(P0) is tracked as a per-sample offset: the pocket only ever moves by
// the projections, which subtract the same mean from the offset.
// The two marks of a row are independent (the edit chain, cmdgen_edit_chain: hold the types and re-place the points, or the
// reverse); cmdgen_inpaint_chain sets both from its one mask.  An edit chain that starts below t = T begins at k_edit_start's
// z ~ q(z_start | K) instead of k_chain_init's z_T and walks the ops from there.
//
// Draws.  Injected noise is [n_draws][Nl][3+P] in call order: draw 0 (z_T or z_start), per op A, B and C if the op jumps, then the
// decode draw; the op table (InpaintBuf::iop) holds the row of each.  Philox draws are keyed by the sample's global pocket
// id as in kernels_ddpm.hip, with the draw counter
//   z_T: 0     A of op i: 1 + i     decode: 1 + n_steps     B of op i: 2 + n_steps + i     C of op i: 2 + 2 n_steps + i
// so with resamplings = jump_length = 1 (n_steps = K) z_T, every A draw and the decode draw are those of
// cmdgen_sample_chain's step with the same index, and a sample without fixed rows follows its trajectory bit for bit.
// Built with -ffp-contract=off; the posterior update and the projection use k_step_count's expressions and sum orders.
#include "cmdgen_sampler.h"

namespace {

__device__ __forceinline__ float idraw(const ChainBuf& c, const Layout& lay, int row, int key, int b, int local, int node, int comp,
                                       int ld) {
    if (c.noise) return c.noise[((size_t)row * lay.Nl + node) * ld + comp];
    float z[4];
    philox_normal4(c.seed, (uint32_t)lay.pocket_gid[b], (uint32_t)(lay.pocket_gid[b] >> 32),
                   (uint32_t)key, (uint32_t)(local * 4 + (comp >> 2)), z);
    return z[comp & 3];
}

}  // namespace

// known rows normalised (en_diffusion.py:874-889), the two masks packed as 1 (x held) + 2 (h held), and the pocket offset of
// z_T's frame (k_chain_init has run: c.xh_pocket is the projected, normalised pocket)
__global__ __launch_bounds__(64) void k_inpaint_prep(Layout lay, Dims d, ChainBuf c, InpaintBuf ip,
                                                     const float* __restrict__ phar_x, const float* __restrict__ phar_onehot,
                                                     const float* __restrict__ fix_x, const float* __restrict__ fix_h,
                                                     const float* __restrict__ pocket_x) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b];
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    float* known = const_cast<float*>(ip.known);
    int nfix = 0;
    for (int i = lane; i < nl; i += 64) {
        const float f = (fix_x[pb + i] != 0.f ? 1.f : 0.f) + (fix_h[pb + i] != 0.f ? 2.f : 0.f);
        ip.fix[pb + i] = f;
        nfix += f != 0.f ? 1 : 0;
        float* o = known + (size_t)(pb + i) * ld;
        for (int k = 0; k < 3; ++k) o[k] = phar_x[(size_t)(pb + i) * 3 + k] / d.norm_x;
        for (int k = 0; k < d.P; ++k) o[3 + k] = (phar_onehot[(size_t)(pb + i) * d.P + k] - d.bias_h) / d.norm_h;
    }
    for (int o = 32; o > 0; o >>= 1) nfix += __shfl_xor(nfix, o);
    float off = 0.f;
    if (lane < 3) {
        float s0 = 0.f, s1 = 0.f;
        for (int i = 0; i < np; ++i) {
            s0 += c.xh_pocket[(size_t)(qb + i) * ldq + lane];
            s1 += pocket_x[(size_t)(qb + i) * 3 + lane] / d.norm_x;
        }
        const float cnt = fmaxf((float)np, 1.0f);
        off = s0 / cnt - s1 / cnt;
    }
    const float o0 = __shfl(off, 0), o1 = __shfl(off, 1), o2 = __shfl(off, 2);
    if (lane == 0) ip.poff[b] = make_float4(o0, o1, o2, (float)nfix);
}

// ------------------------------------------------------------------------------------------------------------
// k_edit_start: the start of an edit chain below t = T, in place of k_chain_init + k_inpaint_prep: z ~ q(z_start | K) as
// ConditionalDDPM.forward forms it (conditional_model.py:235-243, noised_representation :158-179).  Both node sets are centred
// on the phar centre of mass of the given rows, z = alpha xh0 + sigma eps_0 over ALL rows (draw 0), then
// remove_mean_batch(z.x, P.x) and the mean-zero check; the expressions and sum orders are those of k_score_init and of
// k_score_step's level formation (kernels_score.hip).  Leaves what k_inpaint_prep leaves: the known rows normalised (NOT
// centred: step B moves them by the pocket offset), the packed masks and the pocket offset of this frame.  One workgroup
// per sample; evaluation 0 counts its own radius graph.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_edit_start(Layout lay, Dims d, ChainBuf c, InpaintBuf ip, float alpha, float sigma,
                                                    const float* __restrict__ phar_x, const float* __restrict__ phar_onehot,
                                                    const float* __restrict__ fix_x, const float* __restrict__ fix_h,
                                                    const float* __restrict__ pocket_x, const float* __restrict__ pocket_onehot) {
    __shared__ float s_mean[3], s_mean2[3];
    __shared__ int s_nfix;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b];
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    float* known = const_cast<float*>(ip.known);
    if (tid == 0) s_nfix = 0;
    if (tid < 3) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += phar_x[(size_t)(pb + i) * 3 + tid] / d.norm_x;      // index order
        s_mean[tid] = s / fmaxf((float)nl, 1.0f);
    }
    __syncthreads();
    const float c0 = s_mean[0], c1 = s_mean[1], c2 = s_mean[2];
    int nfix = 0;
    for (int i = tid; i < nl; i += 256) {
        const size_t g = (size_t)(pb + i);
        const float f = (fix_x[g] != 0.f ? 1.f : 0.f) + (fix_h[g] != 0.f ? 2.f : 0.f);
        ip.fix[g] = f;
        nfix += f != 0.f ? 1 : 0;
        float* o = known + g * ld;
        float* z = c.z_phar + g * ld;
        for (int k = 0; k < 3; ++k) o[k] = phar_x[g * 3 + k] / d.norm_x;
        for (int k = 0; k < d.P; ++k) o[3 + k] = (phar_onehot[g * d.P + k] - d.bias_h) / d.norm_h;
        for (int k = 0; k < ld; ++k) {
            const float x0 = k < 3 ? phar_x[g * 3 + k] / d.norm_x - (k == 0 ? c0 : k == 1 ? c1 : c2) : o[k];
            const float a = alpha * x0;
            z[k] = a + sigma * idraw(c, lay, 0, 0, b, i, pb + i, k, ld);
        }
    }
    if (nfix) atomicAdd(&s_nfix, nfix);
    for (int i = tid; i < np; i += 256) {
        const size_t g = (size_t)(qb + i);
        float* q = c.xh_pocket + g * ldq;
        q[0] = pocket_x[g * 3 + 0] / d.norm_x - c0; q[1] = pocket_x[g * 3 + 1] / d.norm_x - c1; q[2] = pocket_x[g * 3 + 2] / d.norm_x - c2;
        for (int k = 0; k < d.R; ++k) q[3 + k] = (pocket_onehot[g * d.R + k] - d.bias_h) / d.norm_h;
    }
    __syncthreads();
    if (tid < 3) {                                  // phar centre of mass of z, index order (remove_mean_batch :467-475)
        float sum = 0.f;
        for (int i = 0; i < nl; ++i) sum += c.z_phar[(size_t)(pb + i) * ld + tid];
        s_mean2[tid] = sum / fmaxf((float)nl, 1.0f);
    }
    __syncthreads();
    const float m0 = s_mean2[0], m1 = s_mean2[1], m2 = s_mean2[2];
    for (int i = tid; i < nl + np; i += 256) {
        float* p = i < nl ? c.z_phar + (size_t)(pb + i) * ld : c.xh_pocket + (size_t)(qb + i - nl) * ldq;
        p[0] -= m0; p[1] -= m1; p[2] -= m2;
    }
    __syncthreads();
    if (wave == 0) record_com_check(c.check, c.z_phar, ld, pb, nl, 1.0f, lane);           // assert_mean_zero_with_mask
    if (tid < 3) {                                  // com(P) - com(P0), k_inpaint_prep's expressions
        float s0 = 0.f, s1 = 0.f;
        for (int i = 0; i < np; ++i) {
            s0 += c.xh_pocket[(size_t)(qb + i) * ldq + tid];
            s1 += pocket_x[(size_t)(qb + i) * 3 + tid] / d.norm_x;
        }
        const float cnt = fmaxf((float)np, 1.0f);
        reinterpret_cast<float*>(ip.poff + b)[tid] = s0 / cnt - s1 / cnt;
    }
    if (tid == 3) reinterpret_cast<float*>(ip.poff + b)[3] = (float)s_nfix;
}

// ------------------------------------------------------------------------------------------------------------
// k_inpaint_step_count: one op of the schedule (A, B + merge + projection, C; see the top of the file) FUSED with pass 1
// of the next evaluation's radius graph, as k_step_count (kernels_ddpm.hip) does for the plain chain: the graph is
// counted from the final positions of the op, held in LDS.  z_steps / pocket_steps receive z and P after the merge and
// projection (before a jump).  A sample without a mark and an op without a jump run k_step_count's arithmetic; the
// merge takes a row's x columns when bit 1 of its mask is set and its h columns when bit 2 is set.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_inpaint_step_count(Layout lay, Dims d, ChainBuf c, InpaintBuf ip, Work w,
                                                             const float* __restrict__ eps) {
    extern __shared__ float4 s_pos[];               // [max_n] positions of the sample (phar first), then int sdeg[max_n], then z
    int* sdeg = reinterpret_cast<int*>(s_pos + lay.max_n);
    float* s_z = reinterpret_cast<float*>(sdeg + lay.max_n);      // [nl * ld]
    __shared__ float s_mean[3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6, nt = blockDim.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b], n = nl + np;
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    const int step = c.state->step - 1;             // index of this op (k_readout has counted the evaluation)
    const float4 cf = c.coef[step];
    const float4 cf2 = ip.coef2[step];
    const int4 io = ip.iop[step];
    const float4 off0 = ip.poff[b];
    const bool merge = off0.w > 0.f;
    const bool nan_reset = *w.nan_flag != 0;
    float* zg = c.z_phar + (size_t)pb * ld;
    const float* eg = eps + (size_t)pb * ld;
    const int cnt = nl * ld;
    for (int idx = tid; idx < cnt; idx += nt) s_z[idx] = zg[idx];
    for (int i = tid; i < np; i += nt) {
        const float* q = c.xh_pocket + (size_t)(qb + i) * ldq;
        s_pos[nl + i] = make_float4(q[0], q[1], q[2], 0.f);
    }
    __syncthreads();
    if (wave == 0) record_com_check(c.check + 2 * (1 + step), s_z, ld, 0, nl, 1.0f, lane);   // z_t, the op's input
    __syncthreads();
    // A: the posterior step (k_step_count's expressions)
    for (int idx = tid; idx < cnt; idx += nt) {
        const int i = idx / ld, k = idx - i * ld;
        float e = eg[idx];
        if (nan_reset && k < 3) e = 0.f;
        const float mu = s_z[idx] / cf.x - cf.y * e;
        s_z[idx] = mu + cf.z * idraw(c, lay, io.y, 1 + step, b, i, pb + i, k, ld);
    }
    __syncthreads();
    phar_mean(s_z, nl, ld, tid, s_mean);
    __syncthreads();
    float o0, o1, o2;                               // com(P) - com(P0) of the pocket in LDS
    {
        const float m0 = s_mean[0], m1 = s_mean[1], m2 = s_mean[2];
        sub_mean(s_z, s_pos, nl, n, ld, tid, nt, m0, m1, m2);
        o0 = off0.x - m0; o1 = off0.y - m1; o2 = off0.z - m2;
    }
    __syncthreads();
    // B: the noised known rows moved into the current frame replace the held column groups; then the phar COM projection
    if (merge) {
        const int keyB = 2 + ip.n_steps + step;
        for (int idx = tid; idx < cnt; idx += nt) {
            const int i = idx / ld, k = idx - i * ld;
            if (!((int)ip.fix[pb + i] & (k < 3 ? 1 : 2))) continue;
            float zk = cf2.x * ip.known[(size_t)pb * ld + idx] + cf2.y * idraw(c, lay, io.z, keyB, b, i, pb + i, k, ld);
            if (k < 3) zk = zk + (k == 0 ? o0 : k == 1 ? o1 : o2);
            s_z[idx] = zk;
        }
        __syncthreads();
        phar_mean(s_z, nl, ld, tid, s_mean);
        __syncthreads();
        const float m0 = s_mean[0], m1 = s_mean[1], m2 = s_mean[2];
        sub_mean(s_z, s_pos, nl, n, ld, tid, nt, m0, m1, m2);
        o0 -= m0; o1 -= m1; o2 -= m2;
        __syncthreads();
    }
    // the state after the op (a frame): z and the pocket
    if (c.z_steps)
        for (int idx = tid; idx < cnt; idx += nt) c.z_steps[(size_t)step * lay.Nl * ld + (size_t)pb * ld + idx] = s_z[idx];
    if (c.pocket_steps)
        for (int i = tid; i < np; i += nt) {
            const float4 p = s_pos[nl + i];
            float* o = c.pocket_steps + ((size_t)step * lay.Np + qb + i) * 3;
            o[0] = p.x; o[1] = p.y; o[2] = p.z;
        }
    // C: jump back, z_t' ~ q(z_t' | z_s) (sample_normal_zero_com: draw, then the phar COM projection)
    if (io.x & 1) {
        const int keyC = 2 + 2 * ip.n_steps + step;
        for (int idx = tid; idx < cnt; idx += nt) {
            const int i = idx / ld, k = idx - i * ld;
            const float mu = cf2.z * s_z[idx];
            s_z[idx] = mu + cf2.w * idraw(c, lay, io.w, keyC, b, i, pb + i, k, ld);
        }
        __syncthreads();
        phar_mean(s_z, nl, ld, tid, s_mean);
        __syncthreads();
        const float m0 = s_mean[0], m1 = s_mean[1], m2 = s_mean[2];
        sub_mean(s_z, s_pos, nl, n, ld, tid, nt, m0, m1, m2);
        o0 -= m0; o1 -= m1; o2 -= m2;
        __syncthreads();
    }
    // the new state, and the inputs of the next evaluation
    for (int i = tid; i < n; i += nt) {
        float4 p;
        if (i < nl) {
            const float* z = s_z + i * ld;
            p = make_float4(z[0], z[1], z[2], 0.f);
            w.X0[pb + i] = p;
            for (int l = 0; l < d.L; ++l) w.ACC[(size_t)l * lay.Nm + pb + i] = make_float4(0.f, 0.f, 0.f, 0.f);
            s_pos[i] = p;
        } else {
            p = s_pos[i];
            float* q = c.xh_pocket + (size_t)(qb + i - nl) * ldq;
            q[0] = p.x; q[1] = p.y; q[2] = p.z;
            w.XP[qb + i - nl] = p;
        }
    }
    for (int idx = tid; idx < cnt; idx += nt) zg[idx] = s_z[idx];
    if (tid == 0) ip.poff[b] = make_float4(o0, o1, o2, off0.w);
    __syncthreads();
    // ---- pass 1 of the radius graph of the NEXT evaluation (as k_edge_count / k_step_count)
    for (int i = wave; i < n; i += nwaves) {
        const float4 pi = s_pos[i];
        int deg = 0, self = 0;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            bool ok = false;
            if (j < n) {
                const float r2 = dist2(pi, s_pos[j]);
                ok = (d.cutoff2 < 0.f) || (r2 <= d.cutoff2);
            }
            const unsigned long long m = __ballot(ok);
            deg += __popcll(m);
            if (i >= j0 && i < j0 + 64) self = (int)((m >> (i - j0)) & 1ull);
        }
        if (lane == 0) { sdeg[i] = deg | (self << 30); w.degL[pb + qb + i] = deg | (self << 30); }
    }
    __syncthreads();
    if (wave == 0) {
        int e = 0, eph = 0, ens = 0, ensq = 0;
        for (int i = lane; i < n; i += 64) {
            const int dg = sdeg[i] & 0x3fffffff; e += dg;
            if (i < nl) { eph += dg; ens += dg - ((sdeg[i] >> 30) & 1); }
            else ensq += dg - ((sdeg[i] >> 30) & 1);
        }
        for (int o = 32; o > 0; o >>= 1) {
            e += __shfl_xor(e, o); eph += __shfl_xor(eph, o); ens += __shfl_xor(ens, o); ensq += __shfl_xor(ensq, o);
        }
        if (lane == 0) { w.pocketE[b] = e; w.pocketEph[b] = eph; w.pocketEns[b] = ens; w.pocketEnsQ[b] = ensq; }
    }
    if (b == 0 && tid == 0) {
        if (nan_reset) atomicAdd(&w.counters[4], 1ull);
        atomicAdd(&w.counters[0], 1ull);                       // evaluations (the one about to run)
        atomicAdd(&w.counters[3], (unsigned long long)lay.N);  // nodes
    }
}

void cmdgen_launch_inpaint_prep(const Layout& lay, const Dims& d, const ChainBuf& c, const InpaintBuf& ip, const float* phx,
                                const float* phoh, const float* fix_x, const float* fix_h, const float* px, hipStream_t s) {
    hipLaunchKernelGGL(k_inpaint_prep, dim3(lay.B), dim3(64), 0, s, lay, d, c, ip, phx, phoh, fix_x, fix_h, px);
}
void cmdgen_launch_edit_start(const Layout& lay, const Dims& d, const ChainBuf& c, const InpaintBuf& ip, float alpha, float sigma,
                              const float* phx, const float* phoh, const float* fix_x, const float* fix_h, const float* px,
                              const float* poh, hipStream_t s) {
    hipLaunchKernelGGL(k_edit_start, dim3(lay.B), dim3(256), 0, s, lay, d, c, ip, alpha, sigma, phx, phoh, fix_x, fix_h, px, poh);
}
void cmdgen_launch_inpaint_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const InpaintBuf& ip, const Work& w,
                                      const float* eps, hipStream_t s) {
    const size_t shm = (size_t)lay.max_n * (sizeof(float4) + sizeof(int)) + (size_t)lay.max_n * (3 + d.P) * sizeof(float);
    hipLaunchKernelGGL(k_inpaint_step_count, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), shm, s, lay, d, c, ip, w, eps);
}
