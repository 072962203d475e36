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
#include "cmdgen_step_parts.h"

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
            z[k] = a + sigma * chain_draw(c, lay, lay.Nl, pb, 0, 0, b, i, k, ld);
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
    extern __shared__ float4 s_pos[];               // StepWg's layout: [max_n] positions of the sample (phar first), then int sdeg[max_n], then z
    __shared__ float s_mean[3];
    const StepWg s = step_wg(lay, d, c, w, s_pos, s_mean);
    const EditRow op = edit_row(ip, s);
    const StepRows r = sample_rows(lay, c, s);
    const float* eg = eps + (size_t)s.pb * s.ld;
    load_sample(s, c);
    edit_op(lay, d, c, ip, w, s, r, op, [&](int idx) { return eg[idx]; }, [](float mu, int, int) { return mu; });
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
    const size_t shm = plan_step_lds(lay.max_n, d.P);
    hipLaunchKernelGGL(k_inpaint_step_count, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), shm, s, lay, d, c, ip, w, eps);
}
