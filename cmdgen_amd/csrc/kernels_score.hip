// kernels_score.hip - the scoring chain (ConditionalDDPM.score, cmdgen_score_chain): the diffusion loss of a GIVEN pharmacophore in
// its pocket at a list of noise levels, one network evaluation per level.  Level k of the list (conditional_model.py:198-320, eval mode) is
//   z_k = alpha_k xh0 + sigma_k eps_k, then remove_mean_batch(z_k.x, pocket.x)            (noised_representation, :158-179)
//   error_k[b] = sum_except_batch((eps_k - net(z_k, t_k))^2)                              (:249-251)
// and at a level with t = 0 also log p(h | z_0) (log_pxh_given_z0_without_constants, :58-106).  xh0 is the normalised input centred on
// the phar centre of mass, the pocket a translated copy; both are made once by k_score_init.  The levels do not depend on each other:
// every z_k is formed from the clean rows and the level's own draw.
//
// One step of the chain is k_score_step + the sampler's evaluation.  k_score_step, one workgroup per sample, reads the level index from
// the device step counter, reduces the PREVIOUS level's (eps - net)^2 from the evaluation's output, forms the NEXT level's z and counts
// pass 1 of its radius graph from the positions it holds in LDS - k_step_count's shape (kernels_ddpm.hip).  k_score_final reduces the last
// level.  The draw of a level is used twice, for z and one step later in the reduction: both read the injected row or regenerate the same
// Philox counter (seed, global pocket id, level, node), so they see the same numbers.
//
// Sums: a node's columns are added in column order, the nodes of a sample in index order (sum_except_batch is a row sum followed by
// index_add_), by one thread - no float atomics, so a level's entry does not depend on the launch shape or on the other levels.
// Built with -ffp-contract=off; the projection uses k_step_count's expressions and sum orders.
// The second half of the file is the same chain for groups of pockets that share the rows and the draws (cmdgen_multi_score_chain).
#include "cmdgen_sampler.h"

namespace {

__device__ __forceinline__ float sdraw(const ChainBuf& c, const Layout& lay, int level, int b, int local, int node, int comp, int ld) {
    if (c.noise) return c.noise[((size_t)level * lay.Nl + node) * ld + comp];
    float z[4];
    philox_normal4(c.seed, (uint32_t)lay.pocket_gid[b], (uint32_t)(lay.pocket_gid[b] >> 32),
                   (uint32_t)level, (uint32_t)(local * 4 + (comp >> 2)), z);
    return z[comp & 3];
}

__device__ __forceinline__ float cdf_std(float x) { return 0.5f * (1.0f + erff(x / 1.41421356237309515f)); }

// Level `lv` of sample b: (eps - net)^2 over all columns and over the x columns, and at a t = 0 level the categorical term, summed
// per node into s_row and then in node index order into the level's output row.  c.z_phar still holds the level's z.
__device__ void reduce_level(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const Work& w,
                             const float* __restrict__ eps, int lv, int b, float* s_row) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int nl = lay.num_phar[b], pb = lay.phar_base[b];
    const int ld = 3 + d.P;
    const float4 cf = c.coef[lv];
    const bool zero = cf.z != 0.f;
    const bool nan_reset = *w.nan_flag != 0;
    const float s0cat = cf.y * d.norm_h;                 // sigma_0 on the integer scale of the one-hot
    for (int i = tid; i < nl; i += nt) {
        const float* o = eps + (size_t)(pb + i) * ld;
        float sx = 0.f;
        for (int k = 0; k < 3; ++k) {
            const float net = nan_reset ? 0.f : o[k];    // the reference's batch-wide reset of the velocity (dynamics.py:129-131)
            const float df = sdraw(c, lay, lv, b, i, pb + i, k, ld) - net;
            sx += df * df;
        }
        float sa = sx;
        for (int k = 3; k < ld; ++k) {
            const float df = sdraw(c, lay, lv, b, i, pb + i, k, ld) - o[k];
            sa += df * df;
        }
        float lph = 0.f;
        if (zero) {
            // log p(h | z_0): the normal around each class integrated over the unit bin, normalised over the classes (k_train_loss's expressions)
            const float* z = c.z_phar + (size_t)(pb + i) * ld + 3;
            const float* oh0 = sc.xh0 + (size_t)(pb + i) * ld + 3;
            float mx = -INFINITY;
            for (int k = 0; k < d.P; ++k) {
                const float ctr = z[k] * d.norm_h + d.bias_h - 1.0f;
                const float lp = logf(cdf_std((ctr + 0.5f) / s0cat) - cdf_std((ctr - 0.5f) / s0cat) + 1e-10f);
                mx = fmaxf(mx, lp);
            }
            float se = 0.f, dot = 0.f, ohs = 0.f;
            for (int k = 0; k < d.P; ++k) {
                const float ctr = z[k] * d.norm_h + d.bias_h - 1.0f;
                const float lp = logf(cdf_std((ctr + 0.5f) / s0cat) - cdf_std((ctr - 0.5f) / s0cat) + 1e-10f);
                se += expf(lp - mx);
                const float oh = oh0[k] * d.norm_h + d.bias_h;      // the normalised one-hot un-normalised again (:83)
                dot += lp * oh; ohs += oh;
            }
            lph = dot - (mx + logf(se)) * ohs;
        }
        s_row[3 * i] = sa; s_row[3 * i + 1] = sx; s_row[3 * i + 2] = lph;
    }
    __syncthreads();
    if (tid < 3) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += s_row[3 * i + tid];        // index order, as index_add_
        sc.out[((size_t)lv * lay.B + b) * SC_COLS + tid] = s;
    }
    if (tid == 3) sc.out[((size_t)lv * lay.B + b) * SC_COLS + SC_RESET] = nan_reset ? 1.f : 0.f;
    if (b == 0 && tid == 0 && nan_reset) atomicAdd(&w.counters[4], 1ull);
    __syncthreads();
}

// reduce_level for the multi-pocket scoring chain (k_multi_score_step), the same expressions and sum orders, for up to two rows in one
// pass over the sample's nodes: row A from the member's own eps rows (own), row B from eps_bar (bar).  The level's draw of an element is
// formed once and serves both differences, the categorical term (it depends on z and the clean rows alone) both rows; the row sums of
// A go to s_a, those of B to s_b, and threads 0 .. 3 / 64 .. 67 add them in node index order into row row_a of out_a / row_b of out_b
// ([rows][SC_COLS]).  xh0 and c.z_phar are read at the sample's own rows.  do_a, do_b are uniform over the workgroup; the caller puts
// a barrier behind it before s_a or s_b is written again.
template <class Own, class Bar, class Draw>
__device__ __forceinline__ void reduce_rows(const Layout& lay, const Dims& d, const ChainBuf& c, const float* xh0, bool nan_reset, int lv, int b,
                                            bool do_a, float* s_a, float* out_a, size_t row_a, Own own,
                                            bool do_b, float* s_b, float* out_b, size_t row_b, Bar bar, Draw draw_of) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int nl = lay.num_phar[b], pb = lay.phar_base[b];
    const int ld = 3 + d.P;
    const float4 cf = c.coef[lv];
    const bool zero = cf.z != 0.f;
    const float s0cat = cf.y * d.norm_h;                 // sigma_0 on the integer scale of the one-hot
    for (int i = tid; i < nl; i += nt) {
        float sxa = 0.f, sxb = 0.f;
        for (int k = 0; k < 3; ++k) {
            const float dr = draw_of(i, k);
            if (do_a) {
                const float net = nan_reset ? 0.f : own(i, k);   // the reference's batch-wide reset of the velocity (dynamics.py:129-131)
                const float df = dr - net;
                sxa += df * df;
            }
            if (do_b) {
                const float net = nan_reset ? 0.f : bar(i, k);
                const float df = dr - net;
                sxb += df * df;
            }
        }
        float saa = sxa, sab = sxb;
        for (int k = 3; k < ld; ++k) {
            const float dr = draw_of(i, k);
            if (do_a) { const float df = dr - own(i, k); saa += df * df; }
            if (do_b) { const float df = dr - bar(i, k); sab += df * df; }
        }
        float lph = 0.f;
        if (zero) {
            // log p(h | z_0): the normal around each class integrated over the unit bin, normalised over the classes (k_train_loss's expressions)
            const float* z = c.z_phar + (size_t)(pb + i) * ld + 3;
            const float* oh0 = xh0 + (size_t)(pb + i) * ld + 3;
            float mx = -INFINITY;
            for (int k = 0; k < d.P; ++k) {
                const float ctr = z[k] * d.norm_h + d.bias_h - 1.0f;
                const float lp = logf(cdf_std((ctr + 0.5f) / s0cat) - cdf_std((ctr - 0.5f) / s0cat) + 1e-10f);
                mx = fmaxf(mx, lp);
            }
            float se = 0.f, dot = 0.f, ohs = 0.f;
            for (int k = 0; k < d.P; ++k) {
                const float ctr = z[k] * d.norm_h + d.bias_h - 1.0f;
                const float lp = logf(cdf_std((ctr + 0.5f) / s0cat) - cdf_std((ctr - 0.5f) / s0cat) + 1e-10f);
                se += expf(lp - mx);
                const float oh = oh0[k] * d.norm_h + d.bias_h;      // the normalised one-hot un-normalised again (:83)
                dot += lp * oh; ohs += oh;
            }
            lph = dot - (mx + logf(se)) * ohs;
        }
        if (do_a) { s_a[3 * i] = saa; s_a[3 * i + 1] = sxa; s_a[3 * i + 2] = lph; }
        if (do_b) { s_b[3 * i] = sab; s_b[3 * i + 1] = sxb; s_b[3 * i + 2] = lph; }
    }
    __syncthreads();
    const int t2 = tid - 64;                             // the second row's sums run on another wave beside the first's
    if (do_a && tid < 3) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += s_a[3 * i + tid];          // index order, as index_add_
        out_a[row_a * SC_COLS + tid] = s;
    }
    if (do_a && tid == 3) out_a[row_a * SC_COLS + SC_RESET] = nan_reset ? 1.f : 0.f;
    if (do_b && t2 >= 0 && t2 < 3) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += s_b[3 * i + t2];
        out_b[row_b * SC_COLS + t2] = s;
    }
    if (do_b && t2 == 3) out_b[row_b * SC_COLS + SC_RESET] = nan_reset ? 1.f : 0.f;
}

// the index of the group whose first member is `first` (GroupTab::group_first is ascending)
__device__ __forceinline__ int group_index(const GroupTab& g, int first) {
    int lo = 0, hi = g.G - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g.group_first[mid] < first) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace

// normalize (en_diffusion.py:874-889), centre both node sets on the phar centre of mass (:235-238), and the two sums of the prior KL
// term (mu_T = alpha_T xh0, :20-56).  The slot keeps the clean rows; ChainBuf::xh_pocket gets the pocket (positions rewritten per level).
__global__ __launch_bounds__(256) void k_score_init(Layout lay, Dims d, ChainBuf c, ScoreBuf sc, float alpha_T,
                                                    const float* __restrict__ phar_x, const float* __restrict__ phar_onehot,
                                                    const float* __restrict__ pocket_x, const float* __restrict__ pocket_onehot,
                                                    float* __restrict__ kl_sums) {
    __shared__ float s_mean[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b];
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    float* xh0 = const_cast<float*>(sc.xh0);
    float* p0 = const_cast<float*>(sc.pocket0);
    if (tid < 3) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += phar_x[(size_t)(pb + i) * 3 + tid] / d.norm_x;      // index order
        s_mean[tid] = s / fmaxf((float)nl, 1.0f);
    }
    __syncthreads();
    const float m0 = s_mean[0], m1 = s_mean[1], m2 = s_mean[2];
    for (int i = tid; i < nl; i += 256) {
        const size_t g = (size_t)(pb + i);
        float* o = xh0 + g * ld;
        o[0] = phar_x[g * 3 + 0] / d.norm_x - m0; o[1] = phar_x[g * 3 + 1] / d.norm_x - m1; o[2] = phar_x[g * 3 + 2] / d.norm_x - m2;
        for (int k = 0; k < d.P; ++k) o[3 + k] = (phar_onehot[g * d.P + k] - d.bias_h) / d.norm_h;
        for (int k = 0; k < ld; ++k) c.z_phar[g * ld + k] = o[k];
    }
    for (int i = tid; i < np; i += 256) {
        const size_t g = (size_t)(qb + i);
        const float x0 = pocket_x[g * 3 + 0] / d.norm_x - m0, x1 = pocket_x[g * 3 + 1] / d.norm_x - m1, x2 = pocket_x[g * 3 + 2] / d.norm_x - m2;
        p0[g * 3 + 0] = x0; p0[g * 3 + 1] = x1; p0[g * 3 + 2] = x2;
        float* q = c.xh_pocket + g * ldq;
        q[0] = x0; q[1] = x1; q[2] = x2;
        for (int k = 0; k < d.R; ++k) q[3 + k] = (pocket_onehot[g * d.R + k] - d.bias_h) / d.norm_h;
    }
    __syncthreads();
    if (tid < 2) {              // 0: x columns, 1: feature columns; row sums added in index order
        float s = 0.f;
        for (int i = 0; i < nl; ++i) {
            const float* o = xh0 + (size_t)(pb + i) * ld;
            float r = 0.f;
            for (int k = tid ? 3 : 0; k < (tid ? ld : 3); ++k) { const float a = alpha_T * o[k]; r += a * a; }
            s += r;
        }
        kl_sums[2 * b + tid] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------
// k_score_step: reduce level (step - 1), form level `step` and count pass 1 of its radius graph.  step = ChainState::step is the number of
// evaluations done, i.e. the index of the level about to be evaluated; FINAL: only the reduction (k_score_final).
// ------------------------------------------------------------------------------------------------------------
template <bool FINAL>
__global__ __launch_bounds__(1024) void k_score_step(Layout lay, Dims d, ChainBuf c, ScoreBuf sc, Work w, const float* __restrict__ eps) {
    extern __shared__ float4 s_pos[];               // [max_n] positions (phar first), int sdeg[max_n], z [max_n * ld], row sums [3 * max_n]
    int* sdeg = reinterpret_cast<int*>(s_pos + lay.max_n);
    float* s_z = reinterpret_cast<float*>(sdeg + lay.max_n);
    const int ld = 3 + d.P, ldq = 3 + d.R;
    float* s_row = s_z + (size_t)lay.max_n * ld;
    __shared__ float s_mean[3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6, nt = blockDim.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b], n = nl + np;
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int lv = c.state->step;
    if (lv > 0) reduce_level(lay, d, c, sc, w, eps, lv - 1, b, s_row);
    if (FINAL || lv >= c.state->K) return;          // (K = the number of levels: the list is never walked past its end)
    const float4 cf = c.coef[lv];
    float* zg = c.z_phar + (size_t)pb * ld;
    const float* x0g = sc.xh0 + (size_t)pb * ld;
    const int cnt = nl * ld;
    for (int idx = tid; idx < cnt; idx += nt) {
        const int i = idx / ld, k = idx - i * ld;
        const float a = cf.x * x0g[idx];
        s_z[idx] = a + cf.y * sdraw(c, lay, lv, b, i, pb + i, k, ld);
    }
    for (int i = tid; i < np; i += nt) {
        const float* q = sc.pocket0 + (size_t)(qb + i) * 3;
        s_pos[nl + i] = make_float4(q[0], q[1], q[2], 0.f);
    }
    __syncthreads();
    if (tid < 3) {                                  // phar centre of mass, index order (remove_mean_batch :467-475)
        float sum = 0.f;
        for (int i = 0; i < nl; ++i) sum += s_z[i * ld + tid];
        s_mean[tid] = sum / fmaxf((float)nl, 1.0f);
    }
    __syncthreads();
    const float m0 = s_mean[0], m1 = s_mean[1], m2 = s_mean[2];
    for (int i = tid; i < n; i += nt) {
        float4 p;
        if (i < nl) {
            float* z = s_z + i * ld;
            z[0] -= m0; z[1] -= m1; z[2] -= m2;
            p = make_float4(z[0], z[1], z[2], 0.f);
            w.X0[pb + i] = p;
            for (int l = 0; l < d.L; ++l) w.ACC[(size_t)l * lay.Nm + pb + i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            p = s_pos[i];
            p.x -= m0; p.y -= m1; p.z -= m2;
            float* q = c.xh_pocket + (size_t)(qb + i - nl) * ldq;
            q[0] = p.x; q[1] = p.y; q[2] = p.z;
            w.XP[qb + i - nl] = p;
        }
        s_pos[i] = p;
    }
    __syncthreads();
    for (int idx = tid; idx < cnt; idx += nt) zg[idx] = s_z[idx];
    if (wave == 0) record_com_check(c.check + 2 * lv, s_z, ld, 0, nl, 1.0f, lane);        // the level's z (assert_mean_zero_with_mask)
    // ---- pass 1 of the radius graph of the level's evaluation (as k_edge_count / k_step_count)
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
        atomicAdd(&w.counters[0], 1ull);                       // evaluations (the one about to run)
        atomicAdd(&w.counters[3], (unsigned long long)lay.N);  // nodes
    }
}

// (The NaN flag read by the reduction was set by the previous level's k_readout; pass 2 of the radius graph of the level formed here
// clears it after this kernel has read it, as in the sampling chain.)

// ------------------------------------------------------------------------------------------------------------
// The multi-pocket scoring chain (cmdgen_multi_score_chain): the scoring chain for GROUPS of consecutive samples ("members", GroupTab)
// that share the clean rows and the draws and differ in their pockets - the variational bound of the sampler whose denoiser is
// eps_bar = sum_m w_m eps_m (kernels_multi.hip).  One workgroup per MEMBER.  Every member keeps its own copy of the group's clean rows
// and of the level's z in its own rows of the [Nl] buffers: both depend on the group's raw rows and draws alone, so the copies are
// bit-identical without a workgroup reading what another one of the same launch writes.  The group's row of a level is reduced by
// its first member from all members' eps rows (combine_eps; nothing writes them in these launches), a member's own row from its own.
// With every M = 1 all values are the scoring chain's, bit for bit.
// ------------------------------------------------------------------------------------------------------------
// k_score_init for a member: the centre is the phar centre of mass of the GROUP's raw rows (phar_x, phar_onehot: [Nu] rows, one copy
// per group), summed with k_score_init's expression; the group's first member writes the group's two sums of the prior KL term.
__global__ __launch_bounds__(256) void k_multi_score_init(Layout lay, Dims d, ChainBuf c, ScoreBuf sc, GroupTab g, float alpha_T,
                                                          const float* __restrict__ phar_x, const float* __restrict__ phar_onehot,
                                                          const float* __restrict__ pocket_x, const float* __restrict__ pocket_onehot,
                                                          float* __restrict__ kl_sums) {
    __shared__ float s_mean[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b];
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b], ub = g.ubase[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    float* xh0 = const_cast<float*>(sc.xh0);
    float* p0 = const_cast<float*>(sc.pocket0);
    if (tid < 3) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += phar_x[(size_t)(ub + i) * 3 + tid] / d.norm_x;      // index order
        s_mean[tid] = s / fmaxf((float)nl, 1.0f);
    }
    __syncthreads();
    const float m0 = s_mean[0], m1 = s_mean[1], m2 = s_mean[2];
    for (int i = tid; i < nl; i += 256) {
        const size_t u = (size_t)(ub + i);
        float* o = xh0 + (size_t)(pb + i) * ld;
        o[0] = phar_x[u * 3 + 0] / d.norm_x - m0; o[1] = phar_x[u * 3 + 1] / d.norm_x - m1; o[2] = phar_x[u * 3 + 2] / d.norm_x - m2;
        for (int k = 0; k < d.P; ++k) o[3 + k] = (phar_onehot[u * d.P + k] - d.bias_h) / d.norm_h;
        for (int k = 0; k < ld; ++k) c.z_phar[(size_t)(pb + i) * ld + k] = o[k];
    }
    for (int i = tid; i < np; i += 256) {
        const size_t q0 = (size_t)(qb + i);
        const float x0 = pocket_x[q0 * 3 + 0] / d.norm_x - m0, x1 = pocket_x[q0 * 3 + 1] / d.norm_x - m1, x2 = pocket_x[q0 * 3 + 2] / d.norm_x - m2;
        p0[q0 * 3 + 0] = x0; p0[q0 * 3 + 1] = x1; p0[q0 * 3 + 2] = x2;
        float* q = c.xh_pocket + q0 * ldq;
        q[0] = x0; q[1] = x1; q[2] = x2;
        for (int k = 0; k < d.R; ++k) q[3 + k] = (pocket_onehot[q0 * d.R + k] - d.bias_h) / d.norm_h;
    }
    __syncthreads();
    if (b == g.first[b] && tid < 2) {   // 0: x columns, 1: feature columns; row sums added in index order
        float s = 0.f;
        for (int i = 0; i < nl; ++i) {
            const float* o = xh0 + (size_t)(pb + i) * ld;
            float r = 0.f;
            for (int k = tid ? 3 : 0; k < (tid ? ld : 3); ++k) { const float a = alpha_T * o[k]; r += a * a; }
            s += r;
        }
        kl_sums[2 * group_index(g, b) + tid] = s;
    }
}

// k_score_step for a member.  The previous level: the member's own row (member_out, optional) from its own eps rows, and by the
// group's first member the group's row from eps_bar, in one pass (reduce_rows); it reads the level's draw again.  Then the next level's z from the member's copy
// of the clean rows and the GROUP's draw, the projection, the member's own pocket, the evaluation's inputs and pass 1 of its graph.
template <bool FINAL>
__global__ __launch_bounds__(1024) void k_multi_score_step(Layout lay, Dims d, ChainBuf c, ScoreBuf sc, GroupTab g, Work w,
                                                           const float* __restrict__ eps, float* __restrict__ member_out) {
    extern __shared__ float4 s_pos[];               // k_score_step's layout: positions, degrees, z, row sums
    int* sdeg = reinterpret_cast<int*>(s_pos + lay.max_n);
    float* s_z = reinterpret_cast<float*>(sdeg + lay.max_n);
    const int ld = 3 + d.P, ldq = 3 + d.R;
    float* s_row = s_z + (size_t)lay.max_n * ld;
    __shared__ float s_mean[3];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = blockDim.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b], n = nl + np;
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int first = g.first[b], M = g.size[b];
    const int lv = c.state->step;
    if (lv > 0) {
        const int pl = lv - 1;
        const bool nan_reset = *w.nan_flag != 0;
        const bool do_a = member_out != nullptr, do_b = b == first;
        if (do_a || do_b)                               // (the z block of LDS is free until the next level is formed: the group row's sums)
            reduce_rows(lay, d, c, sc.xh0, nan_reset, pl, b,
                        do_a, s_row, member_out, (size_t)pl * lay.B + b, [&](int i, int k) { return eps[(size_t)(pb + i) * ld + k]; },
                        do_b, s_z, sc.out, do_b ? (size_t)pl * g.G + group_index(g, first) : 0,
                        [&](int i, int k) { return combine_eps(lay, g, eps, first, M, ld, i * ld + k); },
                        [&](int i, int k) { return draw_group(c, lay, g, pl, b, i, k, ld); });
        if (b == 0 && tid == 0 && nan_reset) atomicAdd(&w.counters[4], 1ull);
        __syncthreads();
    }
    if (FINAL || lv >= c.state->K) return;
    const float4 cf = c.coef[lv];
    float* zg = c.z_phar + (size_t)pb * ld;
    const float* x0g = sc.xh0 + (size_t)pb * ld;
    const int cnt = nl * ld;
    for (int idx = tid; idx < cnt; idx += nt) {
        const int i = idx / ld, k = idx - i * ld;
        const float a = cf.x * x0g[idx];
        s_z[idx] = a + cf.y * draw_group(c, lay, g, lv, b, i, k, ld);
    }
    for (int i = tid; i < np; i += nt) {
        const float* q = sc.pocket0 + (size_t)(qb + i) * 3;
        s_pos[nl + i] = make_float4(q[0], q[1], q[2], 0.f);
    }
    __syncthreads();
    phar_mean(s_z, nl, ld, tid, s_mean);            // index order (remove_mean_batch :467-475)
    __syncthreads();
    const float m0 = s_mean[0], m1 = s_mean[1], m2 = s_mean[2];
    for (int i = tid; i < n; i += nt) {
        float4 p;
        if (i < nl) {
            float* z = s_z + i * ld;
            z[0] -= m0; z[1] -= m1; z[2] -= m2;
            p = make_float4(z[0], z[1], z[2], 0.f);
            w.X0[pb + i] = p;
            for (int l = 0; l < d.L; ++l) w.ACC[(size_t)l * lay.Nm + pb + i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            p = s_pos[i];
            p.x -= m0; p.y -= m1; p.z -= m2;
            float* q = c.xh_pocket + (size_t)(qb + i - nl) * ldq;
            q[0] = p.x; q[1] = p.y; q[2] = p.z;
            w.XP[qb + i - nl] = p;
        }
        s_pos[i] = p;
    }
    __syncthreads();
    for (int idx = tid; idx < cnt; idx += nt) zg[idx] = s_z[idx];
    if (wave == 0) record_com_check(c.check + 2 * lv, s_z, ld, 0, nl, 1.0f, lane);        // the level's z, every member's copy
    count_next_graph(lay, d, w, s_pos, sdeg, b, nl, n, pb, qb);
    if (b == 0 && tid == 0) {
        atomicAdd(&w.counters[0], 1ull);                       // evaluations (the one about to run)
        atomicAdd(&w.counters[3], (unsigned long long)lay.N);  // nodes
    }
}

size_t cmdgen_score_step_lds(const Layout& lay, const Dims& d) {
    return (size_t)lay.max_n * (sizeof(float4) + sizeof(int)) + (size_t)lay.max_n * (3 + d.P + 3) * sizeof(float);
}
void cmdgen_launch_score_init(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, float alpha_T, const float* phx,
                              const float* phoh, const float* px, const float* poh, float* kl_sums, hipStream_t s) {
    hipLaunchKernelGGL(k_score_init, dim3(lay.B), dim3(256), 0, s, lay, d, c, sc, alpha_T, phx, phoh, px, poh, kl_sums);
}
void cmdgen_launch_score_step(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const Work& w, const float* eps,
                              hipStream_t s) {
    hipLaunchKernelGGL(k_score_step<false>, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), cmdgen_score_step_lds(lay, d), s, lay, d, c, sc, w, eps);
}
void cmdgen_launch_score_final(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const Work& w, const float* eps,
                               hipStream_t s) {
    hipLaunchKernelGGL(k_score_step<true>, dim3(lay.B), dim3(256), cmdgen_score_step_lds(lay, d), s, lay, d, c, sc, w, eps);
}
void cmdgen_launch_multi_score_init(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const GroupTab& g, float alpha_T,
                                    const float* phx, const float* phoh, const float* px, const float* poh, float* kl_sums, hipStream_t s) {
    hipLaunchKernelGGL(k_multi_score_init, dim3(lay.B), dim3(256), 0, s, lay, d, c, sc, g, alpha_T, phx, phoh, px, poh, kl_sums);
}
void cmdgen_launch_multi_score_step(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const GroupTab& g, const Work& w,
                                    const float* eps, float* member_out, hipStream_t s) {
    hipLaunchKernelGGL(k_multi_score_step<false>, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), cmdgen_score_step_lds(lay, d), s,
                       lay, d, c, sc, g, w, eps, member_out);                             // as k_score_step
}
void cmdgen_launch_multi_score_final(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const GroupTab& g, const Work& w,
                                     const float* eps, float* member_out, hipStream_t s) {
    hipLaunchKernelGGL(k_multi_score_step<true>, dim3(lay.B), dim3(256), cmdgen_score_step_lds(lay, d), s, lay, d, c, sc, g, w, eps, member_out);
}
