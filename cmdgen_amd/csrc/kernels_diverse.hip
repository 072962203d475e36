// kernels_diverse.hip - diverse sampling (ConditionalDDPM.sample_diverse, cmdgen_diverse_chain): the ancestral sampler of kernels_ddpm.hip with
// a term in the mean of every posterior op that pushes the samples drawn for one pocket apart (particle guidance: Corso et al., 2023).  The
// reference draws its samples independently and has nothing like it; this is the definition (include/cmdgen_hip.h and INTEGRATION.md,
// "Diverse sampling", repeat it; tests/diverse_ref.py is its CPU model).
//
// Sets.  The B samples of the layout are partitioned into S sets of consecutive samples (set_size[S], every size >= 1, summing to B).  A set
// is "the draws for one pocket".  Members may have different numbers of points.  The library does not check that the members' pockets are
// copies of each other: positions are compared in the frame in which the caller gives each sample's pocket, so the term is defined either way.
//
// The chain is cmdgen_sample_chain's: the same init, ops, draws, Philox counters (keyed by pocket_ids), saved steps, decode and CoG fix.  The
// evaluations run their own k_readout (there is no own-velocity form).  One addition is made to the mean of every posterior op t -> s.  With
// z, e, P, P_in, n_x, coef and the guide row (sigma_t, alpha_t) as in the header of kernels_restrain.hip, w the width in Angstrom, k >= 0 the
// strength (dimensionless) and M_a the size of sample a's set:
//   1. Denoised estimate, in the caller's frame.  xhat_ai = n_x (z.x_ai - sigma_t e_ai) / alpha_t, with e = 0 under the NaN guard;
//      shift_a = n_x (com(P_a.x) - com(P_a,in.x / n_x));  y_ai = xhat_ai - shift_a.  (xhat_free and frame_shift of cmdgen_guide_parts.h.)
//   2. Overlap.  o_ai = (1 / (M_a - 1)) sum_{b != a, same set} sum_j exp(-|y_ai - y_bj|^2 / (2 w^2)), overlap_a = sum_i o_ai.  The set's energy
//      is E = k / (M - 1) sum_{a < b} sum_{i, j} exp(.), its gradient g_ai = -(k / ((M_a - 1) w^2)) sum_{b != a} sum_j exp(.) (y_ai - y_bj):
//      smooth everywhere, no threshold and no small-distance rule.
//   3. Displacement.  d_ai = -(n_x coef.z)^2 g_ai in Angstrom; if |d_ai| > max_shift it is scaled back to max_shift.  An op with
//      t / T > guide_below, a sample with M_a = 1 and a call with k = 0 have no displacement: nothing is added, not even a zero.
//   4. Mean.  mu.x_ai = z.x_ai / coef.x - coef.y e_ai + d_ai / n_x.  The h columns, the draw, the COM projection, the saved steps and pass 1 of
//      the next radius graph are exactly those of the plain step.  The decode is not guided.
// Outputs beside the chain's: overlap_out [B], step 2 on the RETURNED rows with shift_a = com(xh_pocket_out_a.x) - n_x com(P_a,in.x / n_x) (0
// where M_a = 1); and, when asked for, op_overlap_out [K][B], step 2 at every op's estimate - computed even when k = 0 or the op is above
// guide_below.
//
// Sums.  For point (a, i) the lanes of one wave walk the set's rows in ascending row order, lane-strided, and skip a's own rows; each lane adds
// its terms in that order and a __shfl_xor butterfly adds the lanes.  overlap_a is the sum of the o_ai in index order by one thread.  No float
// atomics; -ffp-contract=off, expf, IEEE sqrtf and division.  The result agrees with the CPU model within rounding, not bit for bit; two runs
// are identical bit for bit, captured or eager.
//
// Reductions that hold bit for bit on every output, the chain status and the "chain_z" debug read: k = 0, guide_below = 0, and every set of one
// member each give cmdgen_sample_chain's outputs on a handle whose evaluations run their own k_readout (readout_in_coord = 0).  overlap_out is
// still reported under k = 0.
//
// Three launches per op, because a term formed inside the step launch would read the other samples' z and pockets while their workgroups
// rewrite them (k_multi_guide's reason):
//   k_diverse_frame        one workgroup per sample: step 1.  Reads z, eps_tmp, the pocket and nan_flag - nothing in the launch writes any of
//                          them - and writes y [Nl][3].
//   k_diverse_pair         one workgroup per sample a: steps 2-3 for a's points, its set's rows of y (a contiguous row range) through LDS in
//                          tiles of PAIR_TILE rows.  Writes gd [Nl][3] and op_overlap.  Static LDS, whatever max_n is.
//   k_diverse_step_count   k_step_count's arithmetic (step_wg, sample_rows, load_sample, plain_op) with gd / n_x in the mean of guided
//                          sample-ops: the un-grouped twin of k_multi_restrained_step_count.
// A sample-op with nothing to do (M = 1, or unguided with no op_overlap asked for) returns at once from the first two.  After k_chain_final
// the first two run once more, in their output mode, over xh_phar_out / xh_pocket_out: overlap_out.
#include "cmdgen_guide_parts.h"

namespace {

enum { PAIR_TILE = 256, PAIR_THREADS = 1024 };      // rows of y per LDS tile (a multiple of 64: a lane keeps its stride over the tiles); one wave per own point, 16 per pass

// (DiverseOp, diverse_op - what an op runs for a sample - are in cmdgen_guide_parts.h: k_diverse_restrained_step_count of kernels_restrain.hip asks too)

// Step 1 for sample b.  output = false: at the op's input (z, eps, the chain's pocket); output = true: on the returned rows xo [Nl][3+P] and
// po [Np][3+R], which are in Angstrom already.  s_q: [max_n] float4 of dynamic LDS.
template <bool output>
__device__ __forceinline__ void diverse_frame_body(const Layout& lay, const Dims& d, const ChainBuf& c, const DiverseBuf& db, const Work& w,
                                                   const float* __restrict__ rows_in, const float* __restrict__ pocket_in,
                                                   const float* __restrict__ eps, float4* s_q, float* s_shift) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = blockDim.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b], pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    [[maybe_unused]] float4 sa = make_float4(0.f, 0.f, 0.f, 0.f);
    [[maybe_unused]] bool nan_reset = false;
    if constexpr (output) {
        if (db.set_size[b] <= 1) return;
    } else {
        const int step = c.state->step - 1;
        if (!diverse_op(db, b, c.coef[step]).terms) return;
        sa = db.sa[step];
        nan_reset = *w.nan_flag != 0;
    }
    for (int i = tid; i < np; i += nt) {
        const float* q = pocket_in + (size_t)(qb + i) * ldq;
        s_q[i] = make_float4(q[0], q[1], q[2], 0.f);
    }
    __syncthreads();
    if (wave == 0) {
        if constexpr (output) {
            float c0, c1, c2;
            wave_com(s_q, np, lane, c0, c1, c2);
            const float4 pin = db.pin_com[b];
            if (lane == 0) { s_shift[0] = c0 - d.norm_x * pin.x; s_shift[1] = c1 - d.norm_x * pin.y; s_shift[2] = c2 - d.norm_x * pin.z; }
        } else frame_shift(d, db, b, s_q, np, lane, s_shift);
    }
    __syncthreads();
    for (int idx = tid; idx < 3 * nl; idx += nt) {
        const int i = idx / 3, k = idx - 3 * i;
        const size_t at = (size_t)(pb + i) * ld + k;
        float xh;
        if constexpr (output) xh = rows_in[at]; else xh = xhat_free(d, sa, rows_in[at], eps[at], nan_reset);
        db.y[(size_t)pb * 3 + idx] = xh - s_shift[k];
    }
}

// Steps 2-3 for the points of sample a = blockIdx.x.  One wave per own point, nwaves points per pass; per pass the set's rows of y go through the
// two LDS tiles in turn, one barrier per tile (a tile is rewritten two barriers after its last reader).  out: where overlap_a goes.
template <bool output>
__device__ __forceinline__ void diverse_pair_body(const Layout& lay, const Dims& d, const DiverseBuf& db, bool guided, const float4& cf,
                                                  float* __restrict__ out, float (*s_y)[PAIR_TILE * 3]) {
    const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6, nt = blockDim.x;
    const int nl = lay.num_phar[a], pb = lay.phar_base[a];
    const int M = db.set_size[a], row0 = db.set_row0[a], rows = db.set_rows[a];
    const float* __restrict__ y = db.y;
    const float per = (float)(M - 1);
    int it = 0;
    for (int i0 = 0; i0 < nl; i0 += nwaves) {
        const int i = i0 + wave;
        const bool own = i < nl;
        float yx = 0.f, yy = 0.f, yz = 0.f;
        if (own) { const float* p = y + (size_t)(pb + i) * 3; yx = p[0]; yy = p[1]; yz = p[2]; }
        float o = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
        for (int t0 = 0; t0 < rows; t0 += PAIR_TILE, ++it) {
            float* tile = s_y[it & 1];
            const int cnt = min((int)PAIR_TILE, rows - t0);
            const float* src = y + (size_t)(row0 + t0) * 3;
            for (int idx = tid; idx < 3 * cnt; idx += nt) tile[idx] = src[idx];
            __syncthreads();
            if (own)
                for (int r = lane; r < cnt; r += 64) {
                    const int row = row0 + t0 + r;
                    if (row >= pb && row < pb + nl) continue;       // a's own rows
                    const float dx = yx - tile[3 * r], dy = yy - tile[3 * r + 1], dz = yz - tile[3 * r + 2];
                    const float e = expf(-(dx * dx + dy * dy + dz * dz) * db.inv2w2);
                    o += e; gx += e * dx; gy += e * dy; gz += e * dz;
                }
        }
        o = wave_sum(o);
        if constexpr (!output) { gx = wave_sum(gx); gy = wave_sum(gy); gz = wave_sum(gz); }
        if (own && lane == 0) {
            db.po[pb + i] = o / per;
            if constexpr (!output) {
                if (guided) {
                    const float gc = -(db.strength / (per * (db.width * db.width)));        // g = gc * sums
                    const float sd = d.norm_x * cf.z, var = sd * sd;
                    float dx = -var * (gc * gx), dy = -var * (gc * gy), dz = -var * (gc * gz);
                    clip_shift(db.max_shift, dx, dy, dz);
                    float* g = db.gd + (size_t)(pb + i) * 3;
                    g[0] = dx; g[1] = dy; g[2] = dz;
                }
            }
        }
    }
    __syncthreads();                                                // po of this sample, written by this workgroup's lanes
    if (out && tid == 0) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += db.po[pb + i];            // index order
        *out = s;
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_diverse_frame(Layout lay, Dims d, ChainBuf c, DiverseBuf db, Work w, const float* __restrict__ eps) {
    extern __shared__ float4 s_q[];                 // [max_n] pocket atoms of the sample
    __shared__ float s_shift[3];
    diverse_frame_body<false>(lay, d, c, db, w, c.z_phar, c.xh_pocket, eps, s_q, s_shift);
}
__global__ __launch_bounds__(256) void k_diverse_frame_out(Layout lay, Dims d, ChainBuf c, DiverseBuf db, Work w, const float* __restrict__ xo,
                                                           const float* __restrict__ po) {
    extern __shared__ float4 s_q[];
    __shared__ float s_shift[3];
    diverse_frame_body<true>(lay, d, c, db, w, xo, po, nullptr, s_q, s_shift);
}

__global__ __launch_bounds__(PAIR_THREADS) void k_diverse_pair(Layout lay, Dims d, ChainBuf c, DiverseBuf db) {
    __shared__ float s_y[2][PAIR_TILE * 3];
    const int a = blockIdx.x;
    const int step = c.state->step - 1;
    const float4 cf = c.coef[step];
    const DiverseOp op = diverse_op(db, a, cf);
    float* out = db.op_overlap ? db.op_overlap + (size_t)step * lay.B + a : nullptr;
    if (!op.terms) {                                // uniform over the workgroup
        if (out && threadIdx.x == 0) *out = 0.f;
        return;
    }
    diverse_pair_body<false>(lay, d, db, op.guided, cf, out, s_y);
}
__global__ __launch_bounds__(PAIR_THREADS) void k_diverse_pair_out(Layout lay, Dims d, DiverseBuf db, float* __restrict__ overlap_out) {
    __shared__ float s_y[2][PAIR_TILE * 3];
    const int a = blockIdx.x;
    if (db.set_size[a] <= 1) {
        if (threadIdx.x == 0) overlap_out[a] = 0.f;
        return;
    }
    diverse_pair_body<true>(lay, d, db, false, make_float4(0.f, 0.f, 0.f, 0.f), overlap_out + a, s_y);
}

// k_step_count on the parts of cmdgen_step_parts.h (the LDS layout, sums and count pass of k_multi_step_count for a sample that is its own group)
// with 4. the sample's displacement in the mean
__global__ __launch_bounds__(1024) void k_diverse_step_count(Layout lay, Dims d, ChainBuf c, DiverseBuf db, Work w, const float* __restrict__ eps,
                                                            const float* __restrict__ gd) {
    extern __shared__ float4 s_pos[];               // StepWg's layout: [max_n] positions of the sample (phar first), then int sdeg[max_n], then z
    __shared__ float s_mean[3];
    const StepWg s = step_wg(lay, d, c, w, s_pos, s_mean);
    const StepRows r = sample_rows(lay, c, s);
    const bool guided = diverse_op(db, s.b, s.cf).guided;           // k_diverse_pair's, which then wrote the sample's d
    const float* eg = eps + (size_t)s.pb * s.ld;
    load_sample(s, c);
    plain_op(lay, d, c, w, s, r, [&](int idx) { return eg[idx]; },
             [&](float mu, int i, int k) { return guided ? mu + gd[(size_t)(s.pb + i) * 3 + k] / d.norm_x : mu; });
}

void cmdgen_launch_diverse_terms(const Layout& lay, const Dims& d, const ChainBuf& c, const DiverseBuf& db, const Work& w, const float* eps,
                                 hipStream_t s) {
    const size_t shm_frame = plan_diverse_frame_lds(lay.max_n);
    hipLaunchKernelGGL(k_diverse_frame, dim3(lay.B), dim3(256), shm_frame, s, lay, d, c, db, w, eps);
    hipLaunchKernelGGL(k_diverse_pair, dim3(lay.B), dim3(PAIR_THREADS), 0, s, lay, d, c, db);
}
void cmdgen_launch_diverse_step(const Layout& lay, const Dims& d, const ChainBuf& c, const DiverseBuf& db, const Work& w, const float* eps,
                                hipStream_t s) {
    cmdgen_launch_diverse_terms(lay, d, c, db, w, eps, s);
    hipLaunchKernelGGL(k_diverse_step_count, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), plan_step_lds(lay.max_n, d.P), s, lay, d, c, db, w,
                       eps, (const float*)db.gd);                   // the block as k_step_count
}
void cmdgen_launch_diverse_overlap(const Layout& lay, const Dims& d, const DiverseBuf& db, const float* xo, const float* po, float* overlap_out,
                                   hipStream_t s) {
    const size_t shm_frame = plan_diverse_frame_lds(lay.max_n);
    hipLaunchKernelGGL(k_diverse_frame_out, dim3(lay.B), dim3(256), shm_frame, s, lay, d, ChainBuf{}, db, Work{}, xo, po);
    hipLaunchKernelGGL(k_diverse_pair_out, dim3(lay.B), dim3(PAIR_THREADS), 0, s, lay, d, db, overlap_out);
}
