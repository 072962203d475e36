// kernels_restrain.hip - sampling steered by geometric restraints (ConditionalDDPM.sample_restrained, cmdgen_restrained_chain): the
// ancestral sampler of kernels_ddpm.hip with a guidance term in the mean of every posterior op.  The reference has nothing like it; this
// is the definition ("Sampling with geometric restraints", repeats it; tests/restraint_ref.py is its CPU model).
//
// The chain is sample_given_pocket's: the same ops, the same draws, the same Philox counters; z_T is k_chain_init's and the decode
// k_chain_final's, which is not guided.  One addition is made to the mean of every posterior op t -> s.  With
//   z     the op's input latent,
//   e     the network's x columns after the NaN guard (zero when the guard reset),
//   P     the current (translated, normalised) pocket,  P_in the caller's pocket,
//   n_x   norm_values[0],
//   coef  the op's step-table row (alpha_ts, sigma2_ts/alpha_ts/sigma_t, sigma_ts*sigma_s/sigma_t, t),
// per sample:
//   1. Denoised estimate.  xhat_i = n_x * (z.x_i - sigma_t * e_i) / alpha_t, in Angstrom, in the chain's current frame; sigma_t and
//      alpha_t are those of the op's t, from a second per-op table beside the step table (RestrainBuf::sa: the host's fp32 evaluation,
//      cmdgen_set_guide_table, or the library's own).
//   2. Frame.  shift = n_x * (com(P.x) - com(P_in.x / n_x)).  A centre c of the caller's frame becomes c + shift; pocket atoms are used
//      where they are, q_a = n_x * P.x_a.
//   3. Energy.  E = sum over restraints of 0.5 * k * v^2, v >= 0 the violation in Angstrom, k >= 0 in 1/Angstrom^2:
//        position(point i, centre c, radius r, k)   v = max(0, |xhat_i - (c + shift)| - r)
//        distance(points i, j, lo, hi, k)           v = max(0, lo - d, d - hi),  d = |xhat_i - xhat_j|
//        exclusion(centre c, radius r, k)           for every point of the sample  v_i = max(0, r - |xhat_i - (c + shift)|)
//        clash(radius r_c, k_c)                     one pair of scalars per call: for every point and every pocket atom of the sample
//                                                   v_ia = max(0, r_c - |xhat_i - q_a|); r_c = 0 turns it off
//      g_i = dE / dxhat_i.  A term whose distance is below 1e-12 A contributes the zero vector.  A point's terms are summed in this
//      order: position, distance and exclusion in list order, then pocket atoms in index order.
//   4. Displacement.  d_i = -scale * (n_x * coef.z)^2 * g_i, in Angstrom: the mean shifted by the op's posterior variance times the
//      gradient (classifier guidance), the gradient taken at xhat with d xhat / d z treated as the identity.  If |d_i| > max_shift,
//      d_i *= max_shift / |d_i|.  An op whose t / T > guide_below has d = 0.
//   5. Mean.  mu.x_i = z.x_i / coef.x - coef.y * e_i + d_i / n_x; the h columns as before.  The draw, the COM projection of z and the
//      pocket, the saved steps and pass 1 of the next radius graph follow exactly as in k_step_count.
// The energy is C1 and the clip is continuous: the term adds no hard threshold; the radius graph's cutoff remains the only one.
// Beside the chain's outputs: per sample the energy E of the FINAL output and its largest violation in Angstrom, evaluated on the
// returned xh_phar / xh_pocket with shift = com(xh_pocket.x) - n_x * com(P_in.x / n_x) (k_restrain_energy); and, when asked for, E at
// xhat of every op.
//
// Reductions that hold bit for bit.  With no restraint on any sample and r_c = 0, or with scale = 0, every output equals
// cmdgen_sample_chain's.  A sample that no restraint touches, an op above guide_below and a chain with scale = 0 run k_step_count's
// arithmetic: nothing is added to their mean, not even a zero.
//
// Sums.  A wave owns a phar point: its lanes walk the sample's restraint records, then the pocket atoms already in LDS, each lane adding
// its terms in ascending order, and a butterfly of __shfl_xor adds the lanes - a fixed order, the same on every run (it is not the index
// order of step 3: the results agree with the CPU model within rounding, not bit for bit).  The pocket's centre of mass is summed the
// same way.  No float atomics anywhere in the guidance.  IEEE sqrtf and division; built with -ffp-contract=off like kernels_ddpm.hip.
//
// The same guidance inside op A of the edit chain (ConditionalDDPM.edit_restrained, cmdgen_restrained_edit_chain): k_restrained_edit_step_count
// below, whose header settles what a held row means to the terms.
#include "cmdgen_guide_parts.h"    // wave_sum, wave_max, wave_com, xhat_free, frame_shift, clip_shift: shared with kernels_diverse.hip

namespace {

struct PointTerm { float gx, gy, gz, e, v; };     // dE / dxhat_i, the point's share of E, its largest violation

// one term of point i: (dx, dy, dz) = xhat_i - the other end, v its violation (> 0), sgn = d v / d dist; count: the term's energy is this point's
__device__ __forceinline__ void add_term(PointTerm& t, float dx, float dy, float dz, float dist, float v, float sgn, float k, bool count) {
    if (dist >= 1e-12f) {
        const float c = sgn * (k * v) / dist;
        t.gx += c * dx; t.gy += c * dy; t.gz += c * dz;
    }
    if (count) { t.e += 0.5f * k * (v * v); t.v = fmaxf(t.v, v); }
}

// Steps 3 of point i, by the whole wave: the sample's records r0 .. r1-1 over the lanes, then its np pocket atoms s_q[0 .. np-1] * qs.
// s_xh: [nl][3] the points in Angstrom; (sx, sy, sz): shift.  Every lane returns the same sums.
__device__ __forceinline__ PointTerm point_terms(const RestrainBuf& rb, int r0, int r1, int i, int np, const float* s_xh, const float4* s_q,
                                                 float qs, float sx, float sy, float sz, int lane) {
    const float xi = s_xh[3 * i], yi = s_xh[3 * i + 1], zi = s_xh[3 * i + 2];
    PointTerm t{0.f, 0.f, 0.f, 0.f, 0.f};
    for (int base = r0; base < r1; base += 64) {
        const int r = base + lane;
        if (r >= r1) continue;
        const RestraintRec q = rb.rec[r];
        if (q.kind == RK_DISTANCE) {
            if (q.i != i && q.j != i) continue;
            const int o = q.i == i ? q.j : q.i;
            const float dx = xi - s_xh[3 * o], dy = yi - s_xh[3 * o + 1], dz = zi - s_xh[3 * o + 2];
            const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
            if (dist < q.a) add_term(t, dx, dy, dz, dist, q.a - dist, -1.f, q.k, q.i == i);
            else if (dist > q.b) add_term(t, dx, dy, dz, dist, dist - q.b, 1.f, q.k, q.i == i);
        } else {
            if (q.kind == RK_POSITION && q.i != i) continue;
            const float dx = xi - (q.c[0] + sx), dy = yi - (q.c[1] + sy), dz = zi - (q.c[2] + sz);
            const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
            if (q.kind == RK_POSITION) { if (dist > q.a) add_term(t, dx, dy, dz, dist, dist - q.a, 1.f, q.k, true); }
            else if (dist < q.a) add_term(t, dx, dy, dz, dist, q.a - dist, -1.f, q.k, true);
        }
    }
    if (rb.clash_r > 0.f) {
        for (int a = lane; a < np; a += 64) {
            const float4 p = s_q[a];
            const float dx = xi - qs * p.x, dy = yi - qs * p.y, dz = zi - qs * p.z;
            const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
            if (dist < rb.clash_r) add_term(t, dx, dy, dz, dist, rb.clash_r - dist, -1.f, rb.clash_k, true);
        }
    }
    t.gx = wave_sum(t.gx); t.gy = wave_sum(t.gy); t.gz = wave_sum(t.gz); t.e = wave_sum(t.e); t.v = wave_max(t.v);
    return t;
}

// which of steps 1-5 an op runs for the owner (sample or group) of the records r0 .. r1-1: guided - the displacement enters the mean; terms - steps 1-4
// run at all (for the displacement, or for op_energy alone).  Uniform over the workgroup.
struct GuideOp { int r0, r1; bool guided, terms; };
__device__ __forceinline__ GuideOp guide_op(const RestrainBuf& rb, int owner, const float4& cf) {
    const int r0 = rb.rstart[owner], r1 = rb.rstart[owner + 1];
    const bool touched = r1 > r0 || rb.clash_r > 0.f;
    const bool guided = touched && rb.scale > 0.f && cf.w <= rb.guide_below;
    return GuideOp{r0, r1, guided, touched && (guided || rb.op_energy != nullptr)};
}

// 1. xhat of a row, one x column, in Angstrom: free - xhat_free (cmdgen_guide_parts.h); held (the edit chains) - the row's given position K
// moved into the current frame
__device__ __forceinline__ float xhat_held(const Dims& d, float known, float shift) { return d.norm_x * known + shift; }

// 2. shift: frame_shift (cmdgen_guide_parts.h)

// 4. the displacement of a point from its gradient sums -> o[0 .. 2]
__device__ __forceinline__ void point_shift(const RestrainBuf& rb, const Dims& d, const float4& cf, float gx, float gy, float gz, float* o) {
    const float sd = d.norm_x * cf.z, var = sd * sd;
    float dx = -rb.scale * var * gx, dy = -rb.scale * var * gy, dz = -rb.scale * var * gz;
    clip_shift(rb.max_shift, dx, dy, dz);
    o[0] = dx; o[1] = dy; o[2] = dz;
}

// 3. / 4. of a sample whose xhat, pocket (s_q) and shift stand in LDS: a wave per point -> s_d [nl][3], s_e [nl]
__device__ __forceinline__ void sample_points(const RestrainBuf& rb, const Dims& d, const float4& cf, const GuideOp& go, int nl, int np, const float* s_xh,
                                              const float4* s_q, const float* s_shift, float* s_d, float* s_e) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const float sx = s_shift[0], sy = s_shift[1], sz = s_shift[2];
    for (int i = wave; i < nl; i += nwaves) {
        const PointTerm t = point_terms(rb, go.r0, go.r1, i, np, s_xh, s_q, d.norm_x, sx, sy, sz, lane);
        if (lane == 0) { point_shift(rb, d, cf, t.gx, t.gy, t.gz, s_d + 3 * i); s_e[i] = t.e; }
    }
    __syncthreads();
}

// E at xhat of this op: the points' shares s_e[0 .. nl-1] in index order (one thread)
__device__ __forceinline__ void store_op_energy(const RestrainBuf& rb, size_t slot, const float* s_e, int nl) {
    float e = 0.f;
    for (int i = 0; i < nl; ++i) e += s_e[i];
    rb.op_energy[slot] = e;
}

}  // namespace

// com(P_in.x / n_x) per sample, index order (scatter_mean of the normalised input pocket)
__global__ __launch_bounds__(64) void k_restrain_prep(Layout lay, Dims d, RestrainBuf rb, const float* __restrict__ pocket_x) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int np = lay.num_pocket[b], qb = lay.pocket_base[b];
    if (lane < 3) {
        float s = 0.f;
        for (int i = 0; i < np; ++i) s += pocket_x[(size_t)(qb + i) * 3 + lane] / d.norm_x;
        reinterpret_cast<float*>(rb.pin_com + b)[lane] = s / fmaxf((float)np, 1.0f);
    }
    if (lane == 3) reinterpret_cast<float*>(rb.pin_com + b)[3] = 0.f;
}

// ------------------------------------------------------------------------------------------------------------
// k_restrained_step_count: k_step_count (kernels_ddpm.hip; both of its forms, own_vel as there) with steps 1-5 of the header between the
// loads and the posterior mean.  xhat, the displacement and the points' energy terms live in LDS behind s_z / s_vel.  A sample-op that is
// not guided (no restraint on the sample and no clash term, scale = 0, t / T > guide_below) skips all of it: k_step_count's arithmetic.
// ------------------------------------------------------------------------------------------------------------
template <bool own_vel>
__global__ __launch_bounds__(1024) void k_restrained_step_count(Layout lay, Dims d, ChainBuf c, RestrainBuf rb, Work w,
                                                               const float* __restrict__ eps) {
    extern __shared__ float4 s_pos[];               // [max_n] positions of the sample (phar first), then int sdeg[max_n], then z, vel, xhat, d, e
    int* sdeg = reinterpret_cast<int*>(s_pos + lay.max_n);
    float* s_z = reinterpret_cast<float*>(sdeg + lay.max_n);      // [nl * ld]
    float* s_vel = s_z + (size_t)lay.max_n * (3 + d.P);           // own_vel: [nl][3]
    float* s_xh = s_vel + (size_t)lay.max_n * 3;                  // [nl][3] xhat, Angstrom
    float* s_d = s_xh + (size_t)lay.max_n * 3;                    // [nl][3] displacement, Angstrom
    float* s_e = s_d + (size_t)lay.max_n * 3;                     // [nl] the points' shares of E
    __shared__ float s_mean[3], s_shift[3];
    __shared__ int s_bad[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6, nt = blockDim.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b], n = nl + np;
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    const int step = c.state->step - 1;
    const float4 cf = c.coef[step];
    const float4 sa = rb.sa[step];
    const GuideOp go = guide_op(rb, b, cf);
    float* zg = c.z_phar + (size_t)pb * ld;
    const float* eg = eps + (size_t)pb * ld;
    const int cnt = nl * ld;
    const int flag0 = own_vel ? 0 : *w.nan_flag;
    [[maybe_unused]] VelIn vin[4];
    if constexpr (own_vel) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = tid + u * nt;
            if (r < lay.Nl) vin[u] = readout_vel_in(lay, w, d, r);
        }
    }
    for (int idx = tid; idx < cnt; idx += nt) s_z[idx] = zg[idx];
    for (int i = tid; i < np; i += nt) {
        const float* q = c.xh_pocket + (size_t)(qb + i) * ldq;
        s_pos[nl + i] = make_float4(q[0], q[1], q[2], 0.f);
    }
    if constexpr (own_vel) {              // the batch-global NaN flag, formed by every workgroup for itself (k_step_count)
        int bad = 0;
        auto take = [&](int r, const float4& v) {
            bad |= vel_isnan(v) ? 1 : 0;
            const int i = r - pb;
            if (i >= 0 && i < nl) { s_vel[3 * i] = v.x; s_vel[3 * i + 1] = v.y; s_vel[3 * i + 2] = v.z; }
        };
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = tid + u * nt;
            if (r < lay.Nl) take(r, readout_vel_of(vin[u]));
        }
        for (int r = tid + 4 * nt; r < lay.Nl; r += nt) take(r, readout_vel(lay, w, d, r));
        const bool any = __ballot(bad != 0) != 0ull;
        if (lane == 0) s_bad[wave] = any ? 1 : 0;
    }
    __syncthreads();
    bool nan_reset;
    if constexpr (own_vel) {
        int any = 0;
        for (int k = 0; k < nwaves; ++k) any |= s_bad[k];
        nan_reset = any != 0;
    } else nan_reset = flag0 != 0;
    if (wave == 0) record_com_check(c.check + 2 * (1 + step), s_z, ld, 0, nl, 1.0f, lane);   // z_t, the step's input
    __syncthreads();
    // ---- the guidance (steps 1-4): uniform over the workgroup
    if (go.terms) {
        for (int idx = tid; idx < 3 * nl; idx += nt) {          // 1. xhat
            const int i = idx / 3, k = idx - 3 * i;
            float e;
            if constexpr (own_vel) e = s_vel[idx]; else e = eg[i * ld + k];
            s_xh[idx] = xhat_free(d, sa, s_z[i * ld + k], e, nan_reset);
        }
        if (wave == nwaves - 1) frame_shift(d, rb, b, s_pos + nl, np, lane, s_shift);     // 2. shift
        __syncthreads();
        sample_points(rb, d, cf, go, nl, np, s_xh, s_pos + nl, s_shift, s_d, s_e);      // 3. / 4.
    }
    if (rb.op_energy && tid == 0) store_op_energy(rb, (size_t)step * lay.B + b, s_e, go.terms ? nl : 0);
    // ---- 5. the posterior mean and the draw (k_step_count's expressions)
    for (int idx = tid; idx < cnt; idx += nt) {
        const int i = idx / ld, k = idx - i * ld;
        float e = eg[idx];
        if constexpr (own_vel) { if (k < 3) e = s_vel[3 * i + k]; }
        if (nan_reset && k < 3) e = 0.f;
        float mu = s_z[idx] / cf.x - cf.y * e;
        if (go.guided && k < 3) mu = mu + s_d[3 * i + k] / d.norm_x;
        s_z[idx] = mu + cf.z * chain_draw(c, lay, lay.Nl, pb, 1 + step, 1 + step, b, i, k, ld);
    }
    __syncthreads();
    phar_mean(s_z, nl, ld, tid, s_mean);
    __syncthreads();
    const float m0 = s_mean[0], m1 = s_mean[1], m2 = s_mean[2];
    for (int i = tid; i < n; i += nt) {
        float4 p;
        if (i < nl) {
            float* z = s_z + i * ld;
            z[0] -= m0; z[1] -= m1; z[2] -= m2;
            p = make_float4(z[0], z[1], z[2], 0.f);
            if constexpr (!own_vel) {         // (own_vel: other workgroups are reading both - pass 2 stores them from z_phar)
                w.X0[pb + i] = p;
                for (int l = 0; l < d.L; ++l) w.ACC[(size_t)l * lay.Nm + pb + i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            p = s_pos[i];
            p.x -= m0; p.y -= m1; p.z -= m2;
            float* q = c.xh_pocket + (size_t)(qb + i - nl) * ldq;
            q[0] = p.x; q[1] = p.y; q[2] = p.z;
            w.XP[qb + i - nl] = p;
            if (c.pocket_steps) {
                float* o = c.pocket_steps + ((size_t)step * lay.Np + qb + i - nl) * 3;
                o[0] = p.x; o[1] = p.y; o[2] = p.z;
            }
        }
        s_pos[i] = p;
    }
    __syncthreads();
    for (int idx = tid; idx < cnt; idx += nt) {
        const float v = s_z[idx];
        zg[idx] = v;
        if (c.z_steps) c.z_steps[(size_t)step * lay.Nl * ld + (size_t)pb * ld + idx] = v;
    }
    count_next_graph(lay, d, w, s_pos, sdeg, b, nl, n, pb, qb);
    if (b == 0 && tid == 0) {
        if (nan_reset) atomicAdd(&w.counters[4], 1ull);
        atomicAdd(&w.counters[0], 1ull);                       // evaluations (the one about to run)
        atomicAdd(&w.counters[3], (unsigned long long)lay.N);  // nodes
    }
}

// ------------------------------------------------------------------------------------------------------------
// k_restrain_energy: E and the largest violation of the chain's OUTPUT (after the decode and the drift fix), per sample: the terms of
// step 3 on xh_phar_out / xh_pocket_out (Angstrom), shift = com(xh_pocket_out.x) - n_x * com(P_in.x / n_x).  256 threads per sample.
// k_multi_restrain_energy: the same for a group: the terms of step 3 on the group's returned rows (xh_phar_out, [Nu] rows) against every member's
// returned pocket, shift = com(xh_pocket_out.x of the first member) - n_x * com(P_first,in.x / n_x).  One workgroup of 256 threads per group.
// One body: the owner's records rstart[owner] .. , its nl rows from row0 of xh_phar_out, the returned pockets of members first .. first + M - 1 (a
// sample is its own only member), a member's sums added in member order as k_multi_guide adds them.
// LDS: [max_n] pocket atoms of the member at hand, then xhat [max_n][3], e [max_n], v [max_n].
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void restrain_energy_body(const Layout& lay, const Dims& d, const RestrainBuf& rb, const float* __restrict__ xh_phar_out,
                                                     const float* __restrict__ xh_pocket_out, float* __restrict__ energy_out, int owner, int first,
                                                     int M, int row0, float4* s_q, float* s_shift) {
    float* s_xh = reinterpret_cast<float*>(s_q + lay.max_n);
    float* s_e = s_xh + (size_t)lay.max_n * 3;
    float* s_v = s_e + lay.max_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6, nt = blockDim.x;
    const int nl = lay.num_phar[first];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    const int r0 = rb.rstart[owner], r1 = rb.rstart[owner + 1];
    if (!(r1 > r0 || rb.clash_r > 0.f)) {           // no restraint touches the sample or group
        if (tid == 0) { energy_out[2 * owner] = 0.f; energy_out[2 * owner + 1] = 0.f; }
        return;
    }
    const int Mq = rb.clash_r > 0.f ? M : 1;        // without the clash term only the first member's pocket is read (the shift)
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int m = 0; m < Mq; ++m) {
        const int b = first + m, np = lay.num_pocket[b], qb = lay.pocket_base[b];
        if (m > 0) __syncthreads();
        if (m == 0)
            for (int idx = tid; idx < 3 * nl; idx += nt) { const int i = idx / 3, k = idx - 3 * i; s_xh[idx] = xh_phar_out[(size_t)(row0 + i) * ld + k]; }
        for (int i = tid; i < np; i += nt) {
            const float* q = xh_pocket_out + (size_t)(qb + i) * ldq;
            s_q[i] = make_float4(q[0], q[1], q[2], 0.f);
        }
        __syncthreads();
        if (m == 0) {
            if (wave == 0) {
                float c0, c1, c2;
                wave_com(s_q, np, lane, c0, c1, c2);
                const float4 pin = rb.pin_com[first];
                if (lane == 0) { s_shift[0] = c0 - d.norm_x * pin.x; s_shift[1] = c1 - d.norm_x * pin.y; s_shift[2] = c2 - d.norm_x * pin.z; }
            }
            __syncthreads();
            sx = s_shift[0]; sy = s_shift[1]; sz = s_shift[2];
        }
        for (int i = wave; i < nl; i += nwaves) {
            const PointTerm t = point_terms(rb, m == 0 ? r0 : 0, m == 0 ? r1 : 0, i, np, s_xh, s_q, 1.0f, sx, sy, sz, lane);
            if (lane == 0) {
                if (m == 0) { s_e[i] = t.e; s_v[i] = t.v; }
                else { s_e[i] += t.e; s_v[i] = fmaxf(s_v[i], t.v); }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        float e = 0.f, v = 0.f;
        for (int i = 0; i < nl; ++i) { e += s_e[i]; v = fmaxf(v, s_v[i]); }     // index order
        energy_out[2 * owner] = e; energy_out[2 * owner + 1] = v;
    }
}

__global__ __launch_bounds__(256) void k_restrain_energy(Layout lay, Dims d, RestrainBuf rb, const float* __restrict__ xh_phar_out,
                                                         const float* __restrict__ xh_pocket_out, float* __restrict__ energy_out) {
    extern __shared__ float4 s_q[];
    __shared__ float s_shift[3];
    const int b = blockIdx.x;
    restrain_energy_body(lay, d, rb, xh_phar_out, xh_pocket_out, energy_out, b, b, 1, lay.phar_base[b], s_q, s_shift);
}

__global__ __launch_bounds__(256) void k_multi_restrain_energy(Layout lay, Dims d, GroupTab g, RestrainBuf rb, const float* __restrict__ xh_phar_out,
                                                               const float* __restrict__ xh_pocket_out, float* __restrict__ energy_out) {
    extern __shared__ float4 s_q[];
    __shared__ float s_shift[3];
    const int grp = blockIdx.x, first = g.group_first[grp];
    restrain_energy_body(lay, d, rb, xh_phar_out, xh_pocket_out, energy_out, grp, first, g.size[first], g.ubase[first], s_q, s_shift);
}

// ------------------------------------------------------------------------------------------------------------
// k_restrained_edit_step_count: editing under restraints (ConditionalDDPM.edit_restrained, cmdgen_restrained_edit_chain).  The chain is
// cmdgen_edit_chain's (kernels_inpaint.hip: the same init, op table, draws and Philox counters, B merge, C jump, saved steps and decode);
// this kernel is k_inpaint_step_count with steps 1-5 of this file's header inside op A of every op t -> s, and three points settled:
//   1. Denoised estimate.  A row whose x columns are NOT held (bit 1 of InpaintBuf::fix clear) has the restrained chain's xhat_i.  A row
//      whose x columns ARE held has xhat_i = n_x K_i.x + shift: its given position moved into the current frame, exactly as a restraint
//      centre is (shift is step 2's, from the pocket in LDS) - so a distance restraint between a free and a held point pulls toward the
//      true held position, not toward a noisy estimate of it.
//   2. Displacement.  d_i as in step 4 for rows whose x is not held.  A row whose x is held gets nothing added to its mean, not even a
//      zero (B replaces it); its energy terms still count in E.  A row with only its types held is a free row here.
//   3. Tables.  RestrainBuf::sa has one row per op of the edit plan (n_steps, following the plan's s with its repeats after jumps): the op
//      that goes to level s takes row K - 1 - s of the K-row guide table.  Op C and the decode are never guided.
// Reductions that hold bit for bit on every output, the chain status and the "chain_z" debug read:
//   - no restraint on any sample and r_c = 0, or scale = 0: cmdgen_edit_chain's outputs for the same arguments (start < timesteps,
//     resamplings > 1 and jump_length > 1 included);
//   - no mark in either mask, start = timesteps, resamplings = jump_length = 1: cmdgen_restrained_chain's outputs on a handle whose
//     evaluations use their own k_readout (readout_in_coord = 0), energy_out, op_energy_out, z_steps and pocket_steps included;
//   - a sample that no restraint touches and an op above guide_below run k_inpaint_step_count's arithmetic;
//   - two runs of the same inputs are equal bit for bit (no float atomics in the guidance).
// LDS: k_inpaint_step_count's layout (positions, degrees, z), then xhat, d and e as in k_restrained_step_count.  eps comes from eps_tmp:
// the evaluations are launched as cmdgen_edit_chain launches them (there is no own-velocity form).
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_restrained_edit_step_count(Layout lay, Dims d, ChainBuf c, InpaintBuf ip, RestrainBuf rb, Work w,
                                                                    const float* __restrict__ eps) {
    extern __shared__ float4 s_pos[];               // StepWg's layout ([max_n] positions, phar first, then int sdeg[max_n], then z), then xhat, d, e
    __shared__ float s_mean[3], s_shift[3];
    const StepWg s = step_wg(lay, d, c, w, s_pos, s_mean);
    float* s_xh = s.s_z + (size_t)lay.max_n * (3 + d.P);          // [nl][3] xhat, Angstrom
    float* s_d = s_xh + (size_t)lay.max_n * 3;                    // [nl][3] displacement, Angstrom
    float* s_e = s_d + (size_t)lay.max_n * 3;                     // [nl] the points' shares of E
    const int lane = s.tid & 63, wave = s.tid >> 6, nwaves = s.nt >> 6;
    const EditRow op = edit_row(ip, s);
    const float4 sa = rb.sa[s.step];
    const GuideOp go = guide_op(rb, s.b, s.cf);
    const float* eg = eps + (size_t)s.pb * s.ld;
    load_sample(s, c);
    // ---- the guidance (steps 1-4): uniform over the workgroup
    if (go.terms) {
        if (wave == nwaves - 1) frame_shift(d, rb, s.b, s_pos + s.nl, s.np, lane, s_shift);      // 2. shift
        __syncthreads();                                        // (held rows read the shift)
        for (int idx = s.tid; idx < 3 * s.nl; idx += s.nt) {    // 1. xhat
            const int i = idx / 3, k = idx - 3 * i;
            s_xh[idx] = ((int)ip.fix[s.pb + i] & 1)             // x held (a marked row: only a sample that merges has one)
                            ? xhat_held(d, ip.known[(size_t)(s.pb + i) * s.ld + k], s_shift[k])
                            : xhat_free(d, sa, s.s_z[i * s.ld + k], eg[i * s.ld + k], s.nan_reset);
        }
        __syncthreads();
        sample_points(rb, d, s.cf, go, s.nl, s.np, s_xh, s_pos + s.nl, s_shift, s_d, s_e);      // 3. / 4.
    }
    if (rb.op_energy && s.tid == 0) store_op_energy(rb, (size_t)s.step * lay.B + s.b, s_e, go.terms ? s.nl : 0);
    // op A with 5. the displacement on the rows whose x is not held; B, C (never guided) and the rest as k_inpaint_step_count
    edit_op(lay, d, c, ip, w, s, sample_rows(lay, c, s), op, [&](int idx) { return eg[idx]; },
            [&](float mu, int i, int k) { return go.guided && !((int)ip.fix[s.pb + i] & 1) ? mu + s_d[3 * i + k] / d.norm_x : mu; });
}

// ------------------------------------------------------------------------------------------------------------
// k_diverse_restrained_step_count: diverse sampling UNDER restraints (ConditionalDDPM.sample_diverse_restrained,
// cmdgen_diverse_restrained_chain): both steering terms in one chain.  This is the definition (include/cmdgen_hip.h and INTEGRATION.md,
// "Diverse sampling under restraints", repeat it; tests/diverse_restrained_ref.py is its CPU model).
// What is unchanged.  The chain is cmdgen_sample_chain's: the same init, ops, draws, Philox counters (keyed by pocket_ids), saved steps and
// CoG fix.  The decode is unguided.  The evaluations run their own k_readout, as the diverse chain's do (there is no own-velocity form).
// Per posterior op t -> s both terms are taken at the same point, the denoised estimate of the op's input, and each keeps the definition and
// the scalars of its own chain:
//   1. Restraint term.  Steps 1-4 of this file's header give d^r_i: xhat, the frame shift, E and g from the sample's records and the clash
//      pair, d^r_i = -scale (n_x coef.z)^2 g_i, clipped at the restraint max_shift.  Active for a touched sample (a record on it, or
//      r_c > 0) when scale > 0 and t / T <= guide_below.
//   2. Overlap term.  Steps 1-3 of kernels_diverse.hip's header give d^v_ai from the set's y = xhat - shift, with strength and width, clipped
//      at its own diverse_max_shift.  Active for a sample of a set with M > 1 when strength > 0 and t / T <= diverse_guide_below.
//   3. Mean.  mu.x_i = ((z.x_i / coef.x - coef.y e_i) + d^r_i / n_x) + d^v_i / n_x: the two additions in that order, each made only where its
//      term is active; nothing is added for an inactive term, not even a zero.  The h columns, the draw, the projection, the saved steps and
//      pass 1 of the next radius graph are the plain step's.
// Side outputs, from the parents' own code: energy_out [B][2] and op_energy_out [K][B] exactly as the restrained chain reports them
// (k_restrain_energy; sample_points and store_op_energy below), overlap_out [B] and op_overlap_out [K][B] exactly as the diverse chain reports
// them (k_diverse_frame_out / k_diverse_pair_out; k_diverse_pair).  A per-op output is still computed where its term is inactive but defined.
// Reductions that hold bit for bit on every output, the chain status and the "chain_z" debug read, on a handle whose evaluations run their
// own k_readout (readout_in_coord = 0):
//   - strength = 0, or diverse_guide_below = 0, or every set of one member: cmdgen_restrained_chain's outputs, energy and op_energy included;
//   - scale = 0, or no record on any sample and r_c = 0: cmdgen_diverse_chain's outputs, overlap and op_overlap included;
//   - both at once: cmdgen_sample_chain's outputs.
// Two runs of the same inputs are equal bit for bit, captured or eager (no float atomics in either term; -ffp-contract=off).
// Three launches per op: k_diverse_frame and k_diverse_pair as they are (the pair term stays out of the step launch, whose other workgroups
// rewrite z and the pockets), then this kernel, one workgroup per sample: the restraint term exactly as k_restrained_step_count<false> forms
// it (xhat_free, frame_shift, sample_points), then plain_op with both displacements in the mean.
// LDS: StepWg's layout, then xhat, d and e as in k_restrained_edit_step_count (plan_diverse_restrained_step_lds: 92 B per node at phar_nf 8,
// so a sample of more than 712 nodes is refused).
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_diverse_restrained_step_count(Layout lay, Dims d, ChainBuf c, RestrainBuf rb, DiverseBuf db, Work w,
                                                                       const float* __restrict__ eps, const float* __restrict__ gd) {
    extern __shared__ float4 s_pos[];               // StepWg's layout ([max_n] positions, phar first, then int sdeg[max_n], then z), then xhat, d, e
    __shared__ float s_mean[3], s_shift[3];
    const StepWg s = step_wg(lay, d, c, w, s_pos, s_mean);
    float* s_xh = s.s_z + (size_t)lay.max_n * (3 + d.P);          // [nl][3] xhat, Angstrom
    float* s_d = s_xh + (size_t)lay.max_n * 3;                    // [nl][3] the restraint displacement, Angstrom
    float* s_e = s_d + (size_t)lay.max_n * 3;                     // [nl] the points' shares of E
    const int lane = s.tid & 63, wave = s.tid >> 6, nwaves = s.nt >> 6;
    const StepRows r = sample_rows(lay, c, s);
    const float4 sa = rb.sa[s.step];
    const GuideOp go = guide_op(rb, s.b, s.cf);
    const bool pushed = diverse_op(db, s.b, s.cf).guided;          // k_diverse_pair's, which then wrote the sample's d^v
    const float* eg = eps + (size_t)s.pb * s.ld;
    load_sample(s, c);
    // ---- the restraint term (steps 1-4): uniform over the workgroup
    if (go.terms) {
        for (int idx = s.tid; idx < 3 * s.nl; idx += s.nt) {    // 1. xhat
            const int i = idx / 3, k = idx - 3 * i;
            s_xh[idx] = xhat_free(d, sa, s.s_z[i * s.ld + k], eg[i * s.ld + k], s.nan_reset);
        }
        if (wave == nwaves - 1) frame_shift(d, rb, s.b, s_pos + s.nl, s.np, lane, s_shift);      // 2. shift
        __syncthreads();
        sample_points(rb, d, s.cf, go, s.nl, s.np, s_xh, s_pos + s.nl, s_shift, s_d, s_e);      // 3. / 4.
    }
    if (rb.op_energy && s.tid == 0) store_op_energy(rb, (size_t)s.step * lay.B + s.b, s_e, go.terms ? s.nl : 0);
    // ---- 3. the mean: the restraint displacement, then the overlap displacement, each only where its term is active
    plain_op(lay, d, c, w, s, r, [&](int idx) { return eg[idx]; },
             [&](float mu, int i, int k) {
                 if (go.guided) mu = mu + s_d[3 * i + k] / d.norm_x;
                 if (pushed) mu = mu + gd[(size_t)(s.pb + i) * 3 + k] / d.norm_x;
                 return mu;
             });
}

// ------------------------------------------------------------------------------------------------------------
// The restrained MULTI-POCKET chain (ConditionalDDPM.sample_restrained_given_pockets, cmdgen_multi_restrained_chain): the guidance of this
// file's header on the shared latent of kernels_multi.hip.  The chain is cmdgen_multi_pocket_chain's - the same layout of B member samples
// in G groups, the same init, ops, draws, Philox counters (keyed by group id), decode and CoG re-centring - with steps 1-5 of the header
// in the mean of every posterior op, applied PER GROUP, and these points settled:
//   Restraints belong to a group: RestraintRec::sample is the group index g, point indices are < n_phar[g], centres are given in the
//     common frame in which the caller gives the group's pockets.  RestrainBuf::rstart is [G + 1], op_energy [K][G], energy_out [G][2].
//   1. Denoised estimate.  xhat_i = n_x (z.x_i - sigma_t ebar_i) / alpha_t with ebar = sum_m w_m eps_m, what the step itself uses
//      (combine_eps: m ascending, the first term not added to a zero); its x columns are zero under the batch-wide NaN guard.
//   2. Frame.  shift_g = n_x (com(P_first.x) - com(P_first,in.x / n_x)), from the group's FIRST member, its pocket as it stands at the
//      op's input - the multi-pocket edit chain's precedent (the offset of its step B is the first member's), and what edit_phars_multi
//      moves results back by.
//   3. Clash.  The sum runs over every point of the group and every pocket atom of EVERY member, q_{m,a} = n_x P_m.x_a as it stands at the
//      op's input; unweighted, weight-0 members included: a point must clash with neither pocket.  A point's terms: the group's records and
//      the first member's atoms (point_terms, exactly k_restrained_step_count's sums), then member by member, ascending, the atoms of each
//      further member (point_terms again, without records), the members' sums added in that order.  No float atomics.
//   4. / 5.  d_i, the max_shift clip, guide_below and mu.x_i = z.x_i / coef.x - coef.y ebar_i + d_i / n_x as in the header.  Every member
//      adds the SAME BITS d_i (one copy per group, read from global memory), so the members' copies of z stay bit-identical.
//   The decode is not guided.  energy_out: E and the largest violation of the returned rows against every member's returned pocket, the
//   shift taken from the first member's returned pocket (k_multi_restrain_energy).
// Two launches per op, because a guidance term computed inside the step launch would read the other members' pocket rows while their
// workgroups translate them:
//   k_multi_guide                  one workgroup per GROUP: steps 1-4.  Reads the first member's copy of z, all members' eps rows and all
//                                  members' pockets - nothing in this launch writes any of them - and writes d [Nu][3] and op_energy.
//   k_multi_restrained_step_count  one workgroup per MEMBER: k_multi_step_count with d_i / n_x in the mean.  Reads d, which nothing in
//                                  this launch writes, and otherwise only what k_multi_step_count reads.
// Reductions that hold bit for bit on every output, the chain status and the "chain_z" debug read:
//   - no record on any group and r_c = 0, or scale = 0, or guide_below = 0: cmdgen_multi_pocket_chain's outputs.  A group-op that is not
//     guided (no record on the group while r_c = 0, scale = 0, t / T > guide_below) adds nothing to the mean, not even a zero;
//   - every M_g = 1: cmdgen_restrained_chain's outputs on a handle whose evaluations use their own k_readout (readout_in_coord = 0),
//     energy_out and op_energy_out included;
//   - two runs of the same inputs are equal bit for bit, captured or eager.
// ------------------------------------------------------------------------------------------------------------
namespace {
// the index of the group whose first member is `first` (GroupTab::group_first is ascending)
__device__ __forceinline__ int group_index(const GroupTab& g, int first) {
    int lo = 0, hi = g.G - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (g.group_first[mid] <= first) lo = mid; else hi = mid - 1;
    }
    return lo;
}
}  // namespace

// steps 1-4 for one group, the body of both guide kernels.  LDS: one member's pocket atoms [max_n] float4 at a time (s_q), then xhat [nl][3],
// the gradient sums [nl][3], e [nl].  held: the group has known rows and marks (the edit chain: known [Nu][ld], fix [Nu]) and a row whose x
// columns are held takes its given position in the current frame for xhat; without it the branch is compiled out.
template <bool held>
__device__ __forceinline__ void multi_guide_body(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const RestrainBuf& rb,
                                                 const Work& w, const float* __restrict__ eps, float* __restrict__ gd,
                                                 const float* __restrict__ known, const float* __restrict__ fix, float4* s_q, float* s_shift) {
    float* s_xh = reinterpret_cast<float*>(s_q + lay.max_n);      // [nl][3] xhat, Angstrom
    float* s_g = s_xh + (size_t)lay.max_n * 3;                    // [nl][3] dE / dxhat
    float* s_e = s_g + (size_t)lay.max_n * 3;                     // [nl] the points' shares of E
    const int grp = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6, nt = blockDim.x;
    const int first = g.group_first[grp], M = g.size[first], ub = g.ubase[first];
    const int nl = lay.num_phar[first], pb = lay.phar_base[first];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    const int step = c.state->step - 1;
    const float4 cf = c.coef[step];
    const float4 sa = rb.sa[step];
    const GuideOp go = guide_op(rb, grp, cf);
    if (!go.terms) {                                // uniform over the workgroup
        if (rb.op_energy && tid == 0) rb.op_energy[(size_t)step * g.G + grp] = 0.f;
        return;
    }
    const bool nan_reset = *w.nan_flag != 0;
    const float* zg = c.z_phar + (size_t)pb * ld;   // the first member's copy
    const int Mq = rb.clash_r > 0.f ? M : 1;        // without the clash term only the first member's pocket is read (the shift)
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int m = 0; m < Mq; ++m) {
        const int b = first + m, np = lay.num_pocket[b], qb = lay.pocket_base[b];
        if (m > 0) __syncthreads();                 // every wave is done with the previous member's atoms
        for (int i = tid; i < np; i += nt) {
            const float* q = c.xh_pocket + (size_t)(qb + i) * ldq;
            s_q[i] = make_float4(q[0], q[1], q[2], 0.f);
        }
        if constexpr (!held) {
            if (m == 0)
                for (int idx = tid; idx < 3 * nl; idx += nt) {    // 1. xhat
                    const int i = idx / 3, k = idx - 3 * i;
                    s_xh[idx] = xhat_free(d, sa, zg[i * ld + k], combine_eps(lay, g, eps, first, M, ld, i * ld + k), nan_reset);
                }
        }
        __syncthreads();
        if (m == 0) {
            if (wave == nwaves - 1) frame_shift(d, rb, first, s_q, np, lane, s_shift);     // 2. shift, from the first member
            __syncthreads();
            sx = s_shift[0]; sy = s_shift[1]; sz = s_shift[2];
            if constexpr (held) {                                 // 1. xhat, behind the shift: a row whose x is held is its given position in the current frame
                for (int idx = tid; idx < 3 * nl; idx += nt) {
                    const int i = idx / 3, k = idx - 3 * i;
                    s_xh[idx] = ((int)fix[ub + i] & 1) ? xhat_held(d, known[(size_t)(ub + i) * ld + k], s_shift[k])
                                                       : xhat_free(d, sa, zg[i * ld + k], combine_eps(lay, g, eps, first, M, ld, i * ld + k), nan_reset);
                }
                __syncthreads();
            }
        }
        for (int i = wave; i < nl; i += nwaves) {                 // 3. a wave per point; the same wave owns the point for every member
            const PointTerm t = point_terms(rb, m == 0 ? go.r0 : 0, m == 0 ? go.r1 : 0, i, np, s_xh, s_q, d.norm_x, sx, sy, sz, lane);
            if (lane == 0) {
                if (m == 0) { s_g[3 * i] = t.gx; s_g[3 * i + 1] = t.gy; s_g[3 * i + 2] = t.gz; s_e[i] = t.e; }
                else { s_g[3 * i] += t.gx; s_g[3 * i + 1] += t.gy; s_g[3 * i + 2] += t.gz; s_e[i] += t.e; }
            }
        }
    }
    if (go.guided && lane == 0)                                   // 4. by the lane that holds the point's sums
        for (int i = wave; i < nl; i += nwaves) point_shift(rb, d, cf, s_g[3 * i], s_g[3 * i + 1], s_g[3 * i + 2], gd + (size_t)(ub + i) * 3);
    __syncthreads();
    if (rb.op_energy && tid == 0) store_op_energy(rb, (size_t)step * g.G + grp, s_e, nl);
}

__global__ __launch_bounds__(1024) void k_multi_guide(Layout lay, Dims d, ChainBuf c, GroupTab g, RestrainBuf rb, Work w,
                                                     const float* __restrict__ eps, float* __restrict__ gd) {
    extern __shared__ float4 s_q[];                 // [max_n] pocket atoms of the member at hand, then xhat, the gradient sums, e
    __shared__ float s_shift[3];
    multi_guide_body<false>(lay, d, c, g, rb, w, eps, gd, nullptr, nullptr, s_q, s_shift);
}

// k_multi_step_count (kernels_multi.hip: the same LDS layout, sums and count pass) with 5. the group's displacement in the mean
__global__ __launch_bounds__(1024) void k_multi_restrained_step_count(Layout lay, Dims d, ChainBuf c, GroupTab g, RestrainBuf rb, Work w,
                                                                     const float* __restrict__ eps, const float* __restrict__ gd) {
    extern __shared__ float4 s_pos[];               // StepWg's layout: [max_n] positions of the sample (phar first), then int sdeg[max_n], then z
    __shared__ float s_mean[3];
    const StepWg s = step_wg(lay, d, c, w, s_pos, s_mean);
    const int first = g.first[s.b], M = g.size[s.b];
    const StepRows r = group_rows(g, c, s);
    const bool guided = guide_op(rb, group_index(g, first), s.cf).guided;         // k_multi_guide's, which then wrote the group's d
    load_sample(s, c);
    plain_op(lay, d, c, w, s, r, [&](int idx) { return combine_eps(lay, g, eps, first, M, s.ld, idx); },
             [&](float mu, int i, int k) { return guided ? mu + gd[(size_t)(r.base + i) * 3 + k] / d.norm_x : mu; });
}

// ------------------------------------------------------------------------------------------------------------
// The restrained MULTI-POCKET EDIT chain (ConditionalDDPM.edit_restrained_given_pockets, cmdgen_multi_restrained_edit_chain): all three
// modifiers at once.  The chain is cmdgen_multi_edit_chain's (kernels_multi.hip: the same layout of B member samples in G groups, both
// inits and k_multi_edit_prep, the plan, the op table, the draw rows and the Philox counters keyed by group id, the B merge with the group's
// offset, the C jump, the saved steps, the decode and the CoG re-centring) with the restrained multi-pocket chain's guidance in the mean of
// op A of every op t -> s, once per GROUP, and three points settled as k_restrained_edit_step_count settles them:
//   1. Denoised estimate.  A row of the group whose x columns are NOT held (bit 1 of InpaintBuf::fix[ubase + i] clear) has
//      xhat_i = n_x (z.x_i - sigma_t ebar_i) / alpha_t, ebar = sum_m w_m eps_m (combine_eps), its x columns zero under the batch-wide NaN
//      guard.  A row whose x columns ARE held has xhat_i = n_x K_i.x + shift_g: its given position moved into the current frame, the way a
//      restraint centre is moved.
//   2. Frame.  shift_g = n_x (com(P_first.x) - pin_com[first]), from the group's first member, its pocket as it stands at the op's input:
//      exactly k_multi_guide's, which also covers start < timesteps, where the init has re-centred every pocket on com(K).  Step B keeps
//      using InpaintBuf::poff.
//   3. Displacement.  d_i (the clash over every member's atoms, the order of the sums, the max_shift clip and the guide_below test are
//      k_multi_guide's: one body) enters mu.x_i = z.x_i / coef.x - coef.y ebar_i + d_i / n_x only on rows whose x is not held.  A held-x
//      row gets nothing added, not even a zero (B replaces it); its energy terms still count in E and op_energy.  A row with only its
//      types held is a free row here.  Every member reads the same bits d_i from global memory: the members' copies of z stay bit-identical.
//   4. Tables.  RestrainBuf::sa has one row per op of the edit plan (n_steps rows, repeats after jumps included): the op that goes to level
//      s takes row K - 1 - s of the K-row guide table.  Op C and the decode are never guided.
// Two launches per op, for k_multi_guide's reason (a member's workgroup translates its own pocket during the step):
//   k_multi_edit_guide                    one workgroup per GROUP.  Reads the first member's z, every member's eps rows and pockets and the
//                                         group's known and fix rows - nothing in this launch writes any of them - and writes d [Nu][3]
//                                         and op_energy [n_steps][G].
//   k_multi_restrained_edit_step_count    one workgroup per MEMBER: k_multi_edit_step_count with step 5 in op A.
// k_multi_restrain_energy fills energy_out [G][2] after the decode, unchanged.
// Reductions that hold bit for bit on every output, the chain status and the "chain_z" debug read:
//   - no record on any group and r_c = 0, or scale = 0, or guide_below = 0: cmdgen_multi_edit_chain's outputs for the same arguments
//     (start < timesteps, resamplings > 1 and jump_length > 1 included);
//   - every M_g = 1: cmdgen_restrained_edit_chain's outputs, energy_out and op_energy_out included, with no option set (both chains'
//     evaluations run their own k_readout);
//   - no mark in either mask, start = timesteps, resamplings = jump_length = 1: cmdgen_multi_restrained_chain's outputs;
//   - two runs of the same inputs are equal bit for bit, captured or eager (no float atomics in the guidance).
// LDS: 44 B per node for the guide, k_multi_edit_step_count's 64 B per node (phar_nf = 8) for the step.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_multi_edit_guide(Layout lay, Dims d, ChainBuf c, GroupTab g, RestrainBuf rb, Work w,
                                                          const float* __restrict__ eps, float* __restrict__ gd,
                                                          const float* __restrict__ known /* InpaintBuf::known */,
                                                          const float* __restrict__ fix /* InpaintBuf::fix */) {
    extern __shared__ float4 s_q[];                 // [max_n] pocket atoms of the member at hand, then xhat, the gradient sums, e
    __shared__ float s_shift[3];
    multi_guide_body<true>(lay, d, c, g, rb, w, eps, gd, known, fix, s_q, s_shift);
}

// k_multi_edit_step_count (kernels_multi.hip: the same LDS layout, sums, merge, jump and count pass) with 5. the group's displacement in the
// mean of op A, on the rows whose x is not held
__global__ __launch_bounds__(1024) void k_multi_restrained_edit_step_count(Layout lay, Dims d, ChainBuf c, GroupTab g, InpaintBuf ip,
                                                                          RestrainBuf rb, Work w, const float* __restrict__ eps,
                                                                          const float* __restrict__ gd) {
    extern __shared__ float4 s_pos[];               // StepWg's layout: [max_n] positions of the sample (phar first), then int sdeg[max_n], then z
    __shared__ float s_mean[3];
    const StepWg s = step_wg(lay, d, c, w, s_pos, s_mean);
    const EditRow op = edit_row(ip, s);             // op.off: this member's copy of the group's offset
    const int first = g.first[s.b], M = g.size[s.b];
    const StepRows r = group_rows(g, c, s);
    const bool guided = guide_op(rb, group_index(g, first), s.cf).guided;         // k_multi_edit_guide's, which then wrote the group's d
    load_sample(s, c);
    edit_op(lay, d, c, ip, w, s, r, op, [&](int idx) { return combine_eps(lay, g, eps, first, M, s.ld, idx); },
            [&](float mu, int i, int k) { return guided && !((int)ip.fix[r.base + i] & 1) ? mu + gd[(size_t)(r.base + i) * 3 + k] / d.norm_x : mu; });
}

void cmdgen_launch_restrain_prep(const Layout& lay, const Dims& d, const RestrainBuf& rb, const float* px, hipStream_t s) {
    hipLaunchKernelGGL(k_restrain_prep, dim3(lay.B), dim3(64), 0, s, lay, d, rb, px);
}
void cmdgen_launch_restrained_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const RestrainBuf& rb, const Work& w,
                                         const float* eps, int own_vel, hipStream_t s) {
    const size_t shm = plan_restrained_step_lds(lay.max_n, d.P);
    const dim3 block(lay.max_n > 128 ? 1024 : 256);             // as k_step_count
    if (own_vel) hipLaunchKernelGGL(k_restrained_step_count<true>, dim3(lay.B), block, shm, s, lay, d, c, rb, w, eps);
    else hipLaunchKernelGGL(k_restrained_step_count<false>, dim3(lay.B), block, shm, s, lay, d, c, rb, w, eps);
}
void cmdgen_launch_restrained_edit_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const InpaintBuf& ip, const RestrainBuf& rb,
                                              const Work& w, const float* eps, hipStream_t s) {
    const size_t shm = plan_restrained_edit_step_lds(lay.max_n, d.P);
    hipLaunchKernelGGL(k_restrained_edit_step_count, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), shm, s, lay, d, c, ip, rb, w, eps);
}
void cmdgen_launch_diverse_restrained_step(const Layout& lay, const Dims& d, const ChainBuf& c, const RestrainBuf& rb, const DiverseBuf& db,
                                           const Work& w, const float* eps, hipStream_t s) {
    cmdgen_launch_diverse_terms(lay, d, c, db, w, eps, s);      // k_diverse_frame, k_diverse_pair: gd and op_overlap
    const size_t shm = plan_diverse_restrained_step_lds(lay.max_n, d.P);
    hipLaunchKernelGGL(k_diverse_restrained_step_count, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), shm, s, lay, d, c, rb, db, w, eps,
                       (const float*)db.gd);                    // the block as k_step_count
}
void cmdgen_launch_restrain_energy(const Layout& lay, const Dims& d, const RestrainBuf& rb, const float* xo, const float* po,
                                   float* energy_out, hipStream_t s) {
    const size_t shm = (size_t)lay.max_n * (sizeof(float4) + 5 * sizeof(float));
    hipLaunchKernelGGL(k_restrain_energy, dim3(lay.B), dim3(256), shm, s, lay, d, rb, xo, po, energy_out);
}
void cmdgen_launch_multi_restrained_step(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const RestrainBuf& rb,
                                         const Work& w, const float* eps, float* gd, hipStream_t s) {
    const dim3 block(lay.max_n > 128 ? 1024 : 256);             // as k_multi_step_count
    const size_t shm_guide = (size_t)lay.max_n * (sizeof(float4) + 7 * sizeof(float));
    const size_t shm_step = plan_step_lds(lay.max_n, d.P);
    hipLaunchKernelGGL(k_multi_guide, dim3(g.G), block, shm_guide, s, lay, d, c, g, rb, w, eps, gd);
    hipLaunchKernelGGL(k_multi_restrained_step_count, dim3(lay.B), block, shm_step, s, lay, d, c, g, rb, w, eps, (const float*)gd);
}
void cmdgen_launch_multi_restrained_edit_step(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const InpaintBuf& ip,
                                              const RestrainBuf& rb, const Work& w, const float* eps, float* gd, hipStream_t s) {
    const dim3 block(lay.max_n > 128 ? 1024 : 256);             // as k_multi_guide and k_multi_edit_step_count
    const size_t shm_guide = (size_t)lay.max_n * (sizeof(float4) + 7 * sizeof(float));
    const size_t shm_step = plan_step_lds(lay.max_n, d.P);
    hipLaunchKernelGGL(k_multi_edit_guide, dim3(g.G), block, shm_guide, s, lay, d, c, g, rb, w, eps, gd, ip.known, (const float*)ip.fix);
    hipLaunchKernelGGL(k_multi_restrained_edit_step_count, dim3(lay.B), block, shm_step, s, lay, d, c, g, ip, rb, w, eps, (const float*)gd);
}
void cmdgen_launch_multi_restrain_energy(const Layout& lay, const Dims& d, const GroupTab& g, const RestrainBuf& rb, const float* xo,
                                         const float* po, float* energy_out, hipStream_t s) {
    const size_t shm = (size_t)lay.max_n * (sizeof(float4) + 5 * sizeof(float));
    hipLaunchKernelGGL(k_multi_restrain_energy, dim3(g.G), dim3(256), shm, s, lay, d, g, rb, xo, po, energy_out);
}
