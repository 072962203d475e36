// kernels_multi.hip - the multi-pocket chain (cmdgen_multi_pocket_chain): kernels_ddpm.hip's init, step and decode for groups of
// M consecutive samples ("members") that share ONE latent z and differ in their pockets.  The evaluation between the ops is the
// ordinary one over the B member samples; an op combines the members' eps rows with the group's weights,
//   eps_bar = sum_m w_m eps_m  (m ascending, the first term is not added to a zero),
// and is sample_given_pocket's op on eps_bar otherwise.  One workgroup per MEMBER: every member keeps its own copy of z, reads
// the eps rows of all members of its group (nothing writes them in these launches), combines them in member order and draws with
// the group's key - so the copies stay bit-identical without any synchronisation between workgroups - then translates its own
// pocket and counts its own edges.  Sums run in index order as in kernels_ddpm.hip; with M = 1 every value is that file's, bit for bit.
#include "cmdgen_step_parts.h"

// subtract the centre of mass of the member's z from its z and its pocket (remove_com of kernels_ddpm.hip)
__device__ __forceinline__ void remove_com_member(float* zx, int ld, int pb, int nl, float* px, int ldq, int qb, int np, int lane) {
    float mean = 0.f;
    if (lane < 3) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += zx[(size_t)(pb + i) * ld + lane];
        mean = s / fmaxf((float)nl, 1.0f);
    }
    const float m0 = __shfl(mean, 0), m1 = __shfl(mean, 1), m2 = __shfl(mean, 2);
    for (int i = lane; i < nl; i += 64) {
        float* p = zx + (size_t)(pb + i) * ld;
        p[0] -= m0; p[1] -= m1; p[2] -= m2;
    }
    for (int i = lane; i < np; i += 64) {
        float* p = px + (size_t)(qb + i) * ldq;
        p[0] -= m0; p[1] -= m1; p[2] -= m2;
    }
}

// z_T = [sum_m w_m com(P_m), 0] + noise, then the COM projection of the member's z and pocket.  A member's centre is summed from
// the RAW input (pocket_x[i] / norm_x in index order: the values k_chain_init stores and sums), never from another member's
// normalised rows, which that member's workgroup may still be writing.
__global__ __launch_bounds__(64) void k_multi_init(Layout lay, Dims d, ChainBuf c, GroupTab g,
                                                   const float* __restrict__ pocket_x,
                                                   const float* __restrict__ pocket_onehot) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b];
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    const int first = g.first[b], M = g.size[b];
    for (int i = lane; i < np; i += 64) {
        float* o = c.xh_pocket + (size_t)(qb + i) * ldq;
        for (int k = 0; k < 3; ++k) o[k] = pocket_x[(size_t)(qb + i) * 3 + k] / d.norm_x;
        for (int k = 0; k < d.R; ++k) o[3 + k] = (pocket_onehot[(size_t)(qb + i) * d.R + k] - d.bias_h) / d.norm_h;
    }
    __syncthreads();
    float mu = 0.f;
    if (lane < 3) {
        for (int m = 0; m < M; ++m) {
            const int qm = lay.pocket_base[first + m], npm = lay.num_pocket[first + m];
            float s = 0.f;
            for (int i = 0; i < npm; ++i) s += pocket_x[(size_t)(qm + i) * 3 + lane] / d.norm_x;
            const float com = s / fmaxf((float)npm, 1.0f);
            mu = m == 0 ? g.weight[first] * com : mu + g.weight[first + m] * com;
        }
    }
    const float m0 = __shfl(mu, 0), m1 = __shfl(mu, 1), m2 = __shfl(mu, 2);
    for (int idx = lane; idx < nl * ld; idx += 64) {
        const int i = idx / ld, k = idx % ld;
        const float m = k == 0 ? m0 : k == 1 ? m1 : k == 2 ? m2 : 0.f;
        c.z_phar[(size_t)(pb + i) * ld + k] = m + 1.0f * chain_draw(c, lay, g.Nu, g.ubase[b], 0, 0, b, i, k, ld);
    }
    __syncthreads();
    remove_com_member(c.z_phar, ld, pb, nl, c.xh_pocket, ldq, qb, np, lane);
    __syncthreads();
    record_com_check(c.check, c.z_phar, ld, pb, nl, 1.0f, lane);
}

// the decode of k_chain_final on eps_bar.  Every member decodes its own copy of z in place and moves its own pocket; the group's first
// member writes the group's rows of xh_phar_out.  The checks and the CoG drift are taken from the member's own values (z * norm_x,
// the bits the output holds), so no workgroup reads rows another one writes.
__global__ __launch_bounds__(64) void k_multi_final(Layout lay, Dims d, ChainBuf c, GroupTab g, Work w,
                                                    const float* __restrict__ eps,
                                                    float* __restrict__ xh_phar_out,
                                                    float* __restrict__ xh_pocket_out,
                                                    unsigned int* cog_slot) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b];
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    const int first = g.first[b], M = g.size[b], ub = g.ubase[b];
    const bool writer = b == first;
    const int K = c.state->K;
    const float4 cf = c.coef[K];                    // (sigma_0, alpha_0, sigma_x = exp(gamma_0/2), 0)
    const bool nan_reset = *w.nan_flag != 0;
    if (writer)
        for (int i = lane; i < nl; i += 64) {       // types: argmax of the un-normalised h of z_0
            const float* z = c.z_phar + (size_t)(pb + i) * ld;
            int best = 0; float bv = z[3] * d.norm_h + d.bias_h;
            for (int k = 1; k < d.P; ++k) { const float v = z[3 + k] * d.norm_h + d.bias_h; if (v > bv) { bv = v; best = k; } }
            float* o = xh_phar_out + (size_t)(ub + i) * ld;
            for (int k = 0; k < d.P; ++k) o[3 + k] = (k == best) ? 1.0f : 0.0f;
        }
    __syncthreads();
    for (int idx = lane; idx < nl * ld; idx += 64) {
        const int i = idx / ld, k = idx % ld;
        const size_t o = (size_t)(pb + i) * ld + k;
        float e = combine_eps(lay, g, eps, first, M, ld, idx);
        if (nan_reset && k < 3) e = 0.f;
        const float mu = (1.0f / cf.y) * (c.z_phar[o] - cf.x * e);
        c.z_phar[o] = mu + cf.z * chain_draw(c, lay, g.Nu, ub, 1 + K, 1 + K, b, i, k, ld);
    }
    __syncthreads();
    remove_com_member(c.z_phar, ld, pb, nl, c.xh_pocket, ldq, qb, np, lane);
    __syncthreads();
    if (writer)
        for (int i = lane; i < nl; i += 64) {
            const float* z = c.z_phar + (size_t)(pb + i) * ld;
            float* o = xh_phar_out + (size_t)(ub + i) * ld;
            o[0] = z[0] * d.norm_x; o[1] = z[1] * d.norm_x; o[2] = z[2] * d.norm_x;
        }
    for (int i = lane; i < np; i += 64) {
        const float* q = c.xh_pocket + (size_t)(qb + i) * ldq;
        float* o = xh_pocket_out + (size_t)(qb + i) * ldq;
        o[0] = q[0] * d.norm_x; o[1] = q[1] * d.norm_x; o[2] = q[2] * d.norm_x;
        for (int k = 0; k < d.R; ++k) o[3 + k] = q[3 + k] * d.norm_h + d.bias_h;
    }
    record_com_check(c.check + 2 * (1 + K), c.z_phar, ld, pb, nl, d.norm_x, lane);
    float s = 0.f;
    if (lane < 3) for (int i = 0; i < nl; ++i) s += c.z_phar[(size_t)(pb + i) * ld + lane] * d.norm_x;
    s = fabsf(s);
    s = max_nan(s, max_nan(__shfl(s, 1), __shfl(s, 2)));
    if (lane == 0) atomic_max_pos(cog_slot, s);
    if (b == 0 && lane == 0 && nan_reset) atomicAdd(&w.counters[4], 1ull);
}

// the batch-wide re-centring of k_chain_drift_fix, one workgroup per GROUP: the group's phar rows and every member's pocket
__global__ __launch_bounds__(64) void k_multi_drift_fix(Layout lay, Dims d, GroupTab g, float* __restrict__ xh_phar_out,
                                                        float* __restrict__ xh_pocket_out, const unsigned int* cog_slot) {
    if (!(__uint_as_float(*cog_slot) > 5e-2f)) return;
    const int first = g.group_first[blockIdx.x], lane = threadIdx.x;
    const int nl = lay.num_phar[first], ub = g.ubase[first], M = g.size[first];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    float mean = 0.f;
    if (lane < 3) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += xh_phar_out[(size_t)(ub + i) * ld + lane];
        mean = s / fmaxf((float)nl, 1.0f);
    }
    const float m0 = __shfl(mean, 0), m1 = __shfl(mean, 1), m2 = __shfl(mean, 2);
    __syncthreads();
    for (int i = lane; i < nl; i += 64) {
        float* p = xh_phar_out + (size_t)(ub + i) * ld;
        p[0] -= m0; p[1] -= m1; p[2] -= m2;
    }
    for (int m = 0; m < M; ++m) {
        const int qb = lay.pocket_base[first + m], np = lay.num_pocket[first + m];
        for (int i = lane; i < np; i += 64) {
            float* p = xh_pocket_out + (size_t)(qb + i) * ldq;
            p[0] -= m0; p[1] -= m1; p[2] -= m2;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// k_multi_step_count: k_step_count (kernels_ddpm.hip) on eps_bar - one posterior step of the member's copy of z, fused with pass 1
// of the radius graph of the member's next evaluation.  Same LDS layout, same sums, same count pass; z_steps (one copy of the
// rows per group) is written by the group's first member.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_multi_step_count(Layout lay, Dims d, ChainBuf c, GroupTab g, Work w,
                                                          const float* __restrict__ eps) {
    extern __shared__ float4 s_pos[];               // StepWg's layout: [max_n] positions of the sample (phar first), then int sdeg[max_n], then z
    __shared__ float s_mean[3];
    const StepWg s = step_wg(lay, d, c, w, s_pos, s_mean);
    const int first = g.first[s.b], M = g.size[s.b];
    load_sample(s, c);
    plain_op(lay, d, c, w, s, group_rows(g, c, s), [&](int idx) { return combine_eps(lay, g, eps, first, M, s.ld, idx); },
             [](float mu, int, int) { return mu; });
}

// ------------------------------------------------------------------------------------------------------------
// The multi-pocket EDIT chain (cmdgen_multi_edit_chain): kernels_inpaint.hip's ops A / B / C on the group's shared latent.  An op
// is k_inpaint_step_count's with eps_bar in place of the sample's own eps rows, the group's draws, and the known rows and marks
// held once per group ([Nu] rows, at ubase + i).  The pocket offset of step B is the GROUP's: com(P_first) - com(P0_first) of the
// group's first member, which every member's workgroup computes for itself after the init launch and keeps in its own slot
// (InpaintBuf::poff[b]); from then on it only changes by the means subtracted from z.  So z depends on eps_bar, the draws, the
// known rows and the offset alone, none of which depends on the member that computes them: the copies stay bit-identical, again
// without a workgroup reading what another one of the same launch writes.  With M = 1 every value is kernels_inpaint.hip's, and
// without marks and jumps k_multi_step_count's, bit for bit.
// ------------------------------------------------------------------------------------------------------------
// what k_inpaint_prep leaves, per group: the known rows normalised and the packed marks (one copy per group, written by its first
// member from the raw inputs), and in EVERY member's slot the group's offset and its number of marked rows.  Runs after the init
// launch (k_multi_init or k_multi_edit_start), which has projected the pockets; nothing writes them here.
__global__ __launch_bounds__(64) void k_multi_edit_prep(Layout lay, Dims d, ChainBuf c, GroupTab g, InpaintBuf ip,
                                                        const float* __restrict__ phar_x, const float* __restrict__ phar_onehot,
                                                        const float* __restrict__ fix_x, const float* __restrict__ fix_h,
                                                        const float* __restrict__ pocket_x) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nl = lay.num_phar[b];
    const int first = g.first[b], ub = g.ubase[b];
    const int qf = lay.pocket_base[first], npf = lay.num_pocket[first];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    const bool writer = b == first;
    float* known = const_cast<float*>(ip.known);
    int nfix = 0;
    for (int i = lane; i < nl; i += 64) {
        const float f = (fix_x[ub + i] != 0.f ? 1.f : 0.f) + (fix_h[ub + i] != 0.f ? 2.f : 0.f);
        nfix += f != 0.f ? 1 : 0;
        if (!writer) continue;
        ip.fix[ub + i] = f;
        float* o = known + (size_t)(ub + i) * ld;
        for (int k = 0; k < 3; ++k) o[k] = phar_x[(size_t)(ub + i) * 3 + k] / d.norm_x;
        for (int k = 0; k < d.P; ++k) o[3 + k] = (phar_onehot[(size_t)(ub + i) * d.P + k] - d.bias_h) / d.norm_h;
    }
    for (int o = 32; o > 0; o >>= 1) nfix += __shfl_xor(nfix, o);
    float off = 0.f;
    if (lane < 3) {                                 // k_inpaint_prep's expression on the first member's rows
        float s0 = 0.f, s1 = 0.f;
        for (int i = 0; i < npf; ++i) {
            s0 += c.xh_pocket[(size_t)(qf + i) * ldq + lane];
            s1 += pocket_x[(size_t)(qf + i) * 3 + lane] / d.norm_x;
        }
        const float cnt = fmaxf((float)npf, 1.0f);
        off = s0 / cnt - s1 / cnt;
    }
    const float o0 = __shfl(off, 0), o1 = __shfl(off, 1), o2 = __shfl(off, 2);
    if (lane == 0) ip.poff[b] = make_float4(o0, o1, o2, (float)nfix);
}

// the start of a chain below t = T, in place of k_multi_init (k_edit_start for a group): every pocket of the group centred on the
// centre of mass of the group's given rows, z ~ q(z_start | K) on the group's draw 0 over ALL rows, then the COM projection of the
// member's z and pocket and the mean-zero check.  Reads the raw inputs only; k_multi_edit_prep follows it.
__global__ __launch_bounds__(256) void k_multi_edit_start(Layout lay, Dims d, ChainBuf c, GroupTab g, float alpha, float sigma,
                                                          const float* __restrict__ phar_x, const float* __restrict__ phar_onehot,
                                                          const float* __restrict__ pocket_x, const float* __restrict__ pocket_onehot) {
    __shared__ float s_mean[3], s_mean2[3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b];
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b], ub = g.ubase[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    if (tid < 3) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += phar_x[(size_t)(ub + i) * 3 + tid] / d.norm_x;      // index order
        s_mean[tid] = s / fmaxf((float)nl, 1.0f);
    }
    __syncthreads();
    const float c0 = s_mean[0], c1 = s_mean[1], c2 = s_mean[2];
    for (int i = tid; i < nl; i += 256) {
        const size_t u = (size_t)(ub + i);
        float* z = c.z_phar + (size_t)(pb + i) * ld;
        for (int k = 0; k < ld; ++k) {
            const float x0 = k < 3 ? phar_x[u * 3 + k] / d.norm_x - (k == 0 ? c0 : k == 1 ? c1 : c2)
                                   : (phar_onehot[u * d.P + k - 3] - d.bias_h) / d.norm_h;
            const float a = alpha * x0;
            z[k] = a + sigma * chain_draw(c, lay, g.Nu, ub, 0, 0, b, i, k, ld);
        }
    }
    for (int i = tid; i < np; i += 256) {
        const size_t q0 = (size_t)(qb + i);
        float* q = c.xh_pocket + q0 * ldq;
        q[0] = pocket_x[q0 * 3 + 0] / d.norm_x - c0; q[1] = pocket_x[q0 * 3 + 1] / d.norm_x - c1; q[2] = pocket_x[q0 * 3 + 2] / d.norm_x - c2;
        for (int k = 0; k < d.R; ++k) q[3 + k] = (pocket_onehot[q0 * d.R + k] - d.bias_h) / d.norm_h;
    }
    __syncthreads();
    if (tid < 3) {                                  // phar centre of mass of z, index order
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
    if (wave == 0) record_com_check(c.check, c.z_phar, ld, pb, nl, 1.0f, lane);
}

// k_inpaint_step_count for a member of a group: same LDS layout, same sums, same count pass as the two step kernels it composes;
// z_steps (one copy of the rows per group) is written by the group's first member, pocket_steps by every member.
__global__ __launch_bounds__(1024) void k_multi_edit_step_count(Layout lay, Dims d, ChainBuf c, GroupTab g, InpaintBuf ip, Work w,
                                                                const float* __restrict__ eps) {
    extern __shared__ float4 s_pos[];               // StepWg's layout: [max_n] positions of the sample (phar first), then int sdeg[max_n], then z
    __shared__ float s_mean[3];
    const StepWg s = step_wg(lay, d, c, w, s_pos, s_mean);
    const EditRow op = edit_row(ip, s);             // op.off: this member's copy of the group's offset
    const int first = g.first[s.b], M = g.size[s.b];
    load_sample(s, c);
    edit_op(lay, d, c, ip, w, s, group_rows(g, c, s), op, [&](int idx) { return combine_eps(lay, g, eps, first, M, s.ld, idx); },
            [](float mu, int, int) { return mu; });
}

void cmdgen_launch_multi_init(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const float* px,
                              const float* poh, hipStream_t s) {
    hipLaunchKernelGGL(k_multi_init, dim3(lay.B), dim3(64), 0, s, lay, d, c, g, px, poh);
}
void cmdgen_launch_multi_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const Work& w,
                                    const float* eps, hipStream_t s) {
    const size_t shm = plan_step_lds(lay.max_n, d.P);
    hipLaunchKernelGGL(k_multi_step_count, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), shm, s, lay, d, c, g, w, eps);   // as k_step_count
}
void cmdgen_launch_multi_final(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const Work& w,
                               const float* eps, float* xo, float* po, unsigned int* cog, hipStream_t s) {
    hipLaunchKernelGGL(k_multi_final, dim3(lay.B), dim3(64), 0, s, lay, d, c, g, w, eps, xo, po, cog);
    hipLaunchKernelGGL(k_multi_drift_fix, dim3(g.G), dim3(64), 0, s, lay, d, g, xo, po, (const unsigned int*)cog);
}
void cmdgen_launch_multi_edit_start(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, float alpha, float sigma,
                                    const float* phx, const float* phoh, const float* px, const float* poh, hipStream_t s) {
    hipLaunchKernelGGL(k_multi_edit_start, dim3(lay.B), dim3(256), 0, s, lay, d, c, g, alpha, sigma, phx, phoh, px, poh);
}
void cmdgen_launch_multi_edit_prep(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const InpaintBuf& ip,
                                   const float* phx, const float* phoh, const float* fix_x, const float* fix_h, const float* px,
                                   hipStream_t s) {
    hipLaunchKernelGGL(k_multi_edit_prep, dim3(lay.B), dim3(64), 0, s, lay, d, c, g, ip, phx, phoh, fix_x, fix_h, px);
}
void cmdgen_launch_multi_edit_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const InpaintBuf& ip,
                                         const Work& w, const float* eps, hipStream_t s) {
    const size_t shm = plan_step_lds(lay.max_n, d.P);
    hipLaunchKernelGGL(k_multi_edit_step_count, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), shm, s, lay, d, c, g, ip, w, eps);   // as its parents
}
