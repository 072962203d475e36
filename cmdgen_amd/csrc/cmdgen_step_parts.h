// cmdgen_step_parts.h - the parts the derived chains' step kernels are composed of (kernels_inpaint.hip, kernels_multi.hip, kernels_restrain.hip, kernels_diverse.hip):
// one workgroup per sample, the sample's z and positions in LDS as in k_step_count (kernels_ddpm.hip).  Device code only.  Every part is
// straight-line code that the whole workgroup calls; what differs between the chain kinds enters as arguments:
//   StepRows        the rows the workgroup draws for and where its known rows, marks, displacements and saved z live (per sample, or per group);
//   eps_of(idx)     element idx of the sample's eps rows: its own row, or combine_eps over the members of its group;
//   mean_x(mu, i, k)  what becomes of the mean of op A in x column k of row i: the unguided chains return mu itself, the restrained ones
//                   mu + d_i / n_x on the rows that take a displacement - and mu itself, with NOTHING added, on every other row (the documented
//                   reductions are bit for bit, and -0.0f + 0.0f is not -0.0f).
// The posterior update and the projection use k_step_count's expressions and sum orders (-ffp-contract=off in every unit that includes this).
#pragma once
#include "cmdgen_sampler.h"

struct StepRows {
    int stride;                 // rows per draw: Layout::Nl, or GroupTab::Nu
    int base;                   // the workgroup's first row among them: phar_base[b], or ubase[b]
    float* z_steps;             // this op's frame of those rows, or null: no frames asked for, or another member of the group writes them
};

// the workgroup's sample and the dynamic LDS every step kernel begins with: [max_n] positions of the sample (phar first), then int sdeg[max_n], then z
struct StepWg {
    int b, tid, nt, nl, np, n, pb, qb, ld, ldq, cnt;
    int step;                   // index of this op (k_readout has counted the evaluation)
    float4 cf;                  // the op's row of the step table
    bool nan_reset;
    float4* s_pos; int* sdeg; float* s_z;       // s_z: [nl * ld]
    float* s_mean;              // [3], static
};
__device__ __forceinline__ StepWg step_wg(const Layout& lay, const Dims& d, const ChainBuf& c, const Work& w, float4* s_pos, float* s_mean) {
    StepWg s;
    s.b = blockIdx.x; s.tid = threadIdx.x; s.nt = blockDim.x;
    s.nl = lay.num_phar[s.b]; s.np = lay.num_pocket[s.b]; s.n = s.nl + s.np;
    s.pb = lay.phar_base[s.b]; s.qb = lay.pocket_base[s.b];
    s.ld = 3 + d.P; s.ldq = 3 + d.R; s.cnt = s.nl * s.ld;
    s.step = c.state->step - 1;
    s.cf = c.coef[s.step];
    s.nan_reset = *w.nan_flag != 0;
    s.s_pos = s_pos; s.sdeg = reinterpret_cast<int*>(s_pos + lay.max_n); s.s_z = reinterpret_cast<float*>(s.sdeg + lay.max_n);
    s.s_mean = s_mean;
    return s;
}
// a sample's own rows, and the rows of its group (the group's first member writes their frames)
__device__ __forceinline__ StepRows sample_rows(const Layout& lay, const ChainBuf& c, const StepWg& s) {
    return StepRows{lay.Nl, s.pb, c.z_steps ? c.z_steps + ((size_t)s.step * lay.Nl + s.pb) * s.ld : nullptr};
}
__device__ __forceinline__ StepRows group_rows(const GroupTab& g, const ChainBuf& c, const StepWg& s) {
    const int ub = g.ubase[s.b];
    return StepRows{g.Nu, ub, c.z_steps && s.b == g.first[s.b] ? c.z_steps + ((size_t)s.step * g.Nu + ub) * s.ld : nullptr};
}

// z and the pocket into LDS, then the mean-zero check of z_t, the op's input
__device__ __forceinline__ void load_sample(const StepWg& s, const ChainBuf& c) {
    const float* zg = c.z_phar + (size_t)s.pb * s.ld;
    for (int idx = s.tid; idx < s.cnt; idx += s.nt) s.s_z[idx] = zg[idx];
    for (int i = s.tid; i < s.np; i += s.nt) {
        const float* q = c.xh_pocket + (size_t)(s.qb + i) * s.ldq;
        s.s_pos[s.nl + i] = make_float4(q[0], q[1], q[2], 0.f);
    }
    __syncthreads();
    if ((s.tid >> 6) == 0) record_com_check(c.check + 2 * (1 + s.step), s.s_z, s.ld, 0, s.nl, 1.0f, s.tid & 63);
    __syncthreads();
}

// A: the posterior step (k_step_count's expressions), drawing row `row` with the counter 1 + step
template <class Eps, class MeanX>
__device__ __forceinline__ void op_a(const Layout& lay, const ChainBuf& c, const StepWg& s, const StepRows& r, int row, Eps eps_of, MeanX mean_x) {
    for (int idx = s.tid; idx < s.cnt; idx += s.nt) {
        const int i = idx / s.ld, k = idx - i * s.ld;
        float e = eps_of(idx);
        if (s.nan_reset && k < 3) e = 0.f;
        float mu = s.s_z[idx] / s.cf.x - s.cf.y * e;
        if (k < 3) mu = mean_x(mu, i, k);
        s.s_z[idx] = mu + s.cf.z * chain_draw(c, lay, r.stride, r.base, row, 1 + s.step, s.b, i, k, s.ld);
    }
}

// the phar COM projection of the z just written to LDS, the pocket in LDS and the offset com(P) - com(P0) of that pocket (off.w rides along)
__device__ __forceinline__ void project(const StepWg& s, float4& off) {
    __syncthreads();
    phar_mean(s.s_z, s.nl, s.ld, s.tid, s.s_mean);
    __syncthreads();
    const float m0 = s.s_mean[0], m1 = s.s_mean[1], m2 = s.s_mean[2];
    sub_mean(s.s_z, s.s_pos, s.nl, s.n, s.ld, s.tid, s.nt, m0, m1, m2);
    off.x -= m0; off.y -= m1; off.z -= m2;
    __syncthreads();
}

// B: the noised known rows moved into the current frame replace the held column groups (bit 1 of a row's mark: x, bit 2: h)
__device__ __forceinline__ void op_b(const Layout& lay, const ChainBuf& c, const InpaintBuf& ip, const StepWg& s, const StepRows& r,
                                     const float4& cf2, int row, const float4& off) {
    const int keyB = 2 + ip.n_steps + s.step;
    const float o0 = off.x, o1 = off.y, o2 = off.z;
    for (int idx = s.tid; idx < s.cnt; idx += s.nt) {
        const int i = idx / s.ld, k = idx - i * s.ld;
        if (!((int)ip.fix[r.base + i] & (k < 3 ? 1 : 2))) continue;
        float zk = cf2.x * ip.known[(size_t)r.base * s.ld + idx] + cf2.y * chain_draw(c, lay, r.stride, r.base, row, keyB, s.b, i, k, s.ld);
        if (k < 3) zk = zk + (k == 0 ? o0 : k == 1 ? o1 : o2);
        s.s_z[idx] = zk;
    }
}

// the state after the op (a frame): z where r says, the sample's pocket
__device__ __forceinline__ void save_frame(const Layout& lay, const ChainBuf& c, const StepWg& s, const StepRows& r) {
    if (r.z_steps)
        for (int idx = s.tid; idx < s.cnt; idx += s.nt) r.z_steps[idx] = s.s_z[idx];
    if (c.pocket_steps)
        for (int i = s.tid; i < s.np; i += s.nt) {
            const float4 p = s.s_pos[s.nl + i];
            float* o = c.pocket_steps + ((size_t)s.step * lay.Np + s.qb + i) * 3;
            o[0] = p.x; o[1] = p.y; o[2] = p.z;
        }
}

// C: jump back, z_t' ~ q(z_t' | z_s) (sample_normal_zero_com: this draw, then the projection)
__device__ __forceinline__ void op_c(const Layout& lay, const ChainBuf& c, const InpaintBuf& ip, const StepWg& s, const StepRows& r,
                                     const float4& cf2, int row) {
    const int keyC = 2 + 2 * ip.n_steps + s.step;
    for (int idx = s.tid; idx < s.cnt; idx += s.nt) {
        const int i = idx / s.ld, k = idx - i * s.ld;
        const float mu = cf2.z * s.s_z[idx];
        s.s_z[idx] = mu + cf2.w * chain_draw(c, lay, r.stride, r.base, row, keyC, s.b, i, k, s.ld);
    }
}

// the new state, and the inputs of the next evaluation; ends on the barrier count_next_graph asks for
__device__ __forceinline__ void store_state(const Layout& lay, const Dims& d, const ChainBuf& c, const InpaintBuf& ip, const Work& w, const StepWg& s,
                                            const float4& off) {
    for (int i = s.tid; i < s.n; i += s.nt) {
        float4 p;
        if (i < s.nl) {
            const float* z = s.s_z + i * s.ld;
            p = make_float4(z[0], z[1], z[2], 0.f);
            w.X0[s.pb + i] = p;
            for (int l = 0; l < d.L; ++l) w.ACC[(size_t)l * lay.Nm + s.pb + i] = make_float4(0.f, 0.f, 0.f, 0.f);
            s.s_pos[i] = p;
        } else {
            p = s.s_pos[i];
            float* q = c.xh_pocket + (size_t)(s.qb + i - s.nl) * s.ldq;
            q[0] = p.x; q[1] = p.y; q[2] = p.z;
            w.XP[s.qb + i - s.nl] = p;
        }
    }
    float* zg = c.z_phar + (size_t)s.pb * s.ld;
    for (int idx = s.tid; idx < s.cnt; idx += s.nt) zg[idx] = s.s_z[idx];
    if (s.tid == 0) ip.poff[s.b] = off;
    __syncthreads();
}

// the plain step's second half: the projection of the z just written to LDS and of the pocket, the new state, the inputs of the next evaluation and
// the saved steps (k_step_count's "project, store and save steps")
__device__ __forceinline__ void project_store_plain(const Layout& lay, const Dims& d, const ChainBuf& c, const Work& w, const StepWg& s, const StepRows& r) {
    __syncthreads();
    phar_mean(s.s_z, s.nl, s.ld, s.tid, s.s_mean);  // centre of mass of the new z, index order
    __syncthreads();
    const float m0 = s.s_mean[0], m1 = s.s_mean[1], m2 = s.s_mean[2];
    for (int i = s.tid; i < s.n; i += s.nt) {
        float4 p;
        if (i < s.nl) {
            float* z = s.s_z + i * s.ld;
            z[0] -= m0; z[1] -= m1; z[2] -= m2;
            p = make_float4(z[0], z[1], z[2], 0.f);
            w.X0[s.pb + i] = p;
            for (int l = 0; l < d.L; ++l) w.ACC[(size_t)l * lay.Nm + s.pb + i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            p = s.s_pos[i];
            p.x -= m0; p.y -= m1; p.z -= m2;
            float* q = c.xh_pocket + (size_t)(s.qb + i - s.nl) * s.ldq;
            q[0] = p.x; q[1] = p.y; q[2] = p.z;
            w.XP[s.qb + i - s.nl] = p;
            if (c.pocket_steps) {
                float* o = c.pocket_steps + ((size_t)s.step * lay.Np + s.qb + i - s.nl) * 3;
                o[0] = p.x; o[1] = p.y; o[2] = p.z;
            }
        }
        s.s_pos[i] = p;
    }
    __syncthreads();
    float* zg = c.z_phar + (size_t)s.pb * s.ld;
    for (int idx = s.tid; idx < s.cnt; idx += s.nt) {
        const float v = s.s_z[idx];
        zg[idx] = v;
        if (r.z_steps) r.z_steps[idx] = v;
    }
}

// the batch's counters, by one thread of the launch
__device__ __forceinline__ void count_evaluation(const Layout& lay, const Work& w, const StepWg& s) {
    if (s.b == 0 && s.tid == 0) {
        if (s.nan_reset) atomicAdd(&w.counters[4], 1ull);
        atomicAdd(&w.counters[0], 1ull);                       // evaluations (the one about to run)
        atomicAdd(&w.counters[3], (unsigned long long)lay.N);  // nodes
    }
}

// the op's rows of the edit plan's tables and the offset com(P) - com(P0) the workgroup keeps (off.w: the number of marked rows)
struct EditRow { float4 cf2; int4 io; float4 off; };
__device__ __forceinline__ EditRow edit_row(const InpaintBuf& ip, const StepWg& s) { return EditRow{ip.coef2[s.step], ip.iop[s.step], ip.poff[s.b]}; }

// One op of the edit plan on the loaded sample, as the header of k_inpaint_step_count (kernels_inpaint.hip) defines it: A and its projection, B and
// its projection on a sample with a mark, the saved frame, C and its projection where the plan jumps back, then the new state, pass 1 of the next
// evaluation's radius graph from the final positions in LDS, and the counters.
template <class Eps, class MeanX>
__device__ __forceinline__ void edit_op(const Layout& lay, const Dims& d, const ChainBuf& c, const InpaintBuf& ip, const Work& w, const StepWg& s,
                                        const StepRows& r, const EditRow& op, Eps eps_of, MeanX mean_x) {
    float4 off = op.off;
    op_a(lay, c, s, r, op.io.y, eps_of, mean_x);
    project(s, off);
    if (off.w > 0.f) {                              // a sample with a mark
        op_b(lay, c, ip, s, r, op.cf2, op.io.z, off);
        project(s, off);
    }
    save_frame(lay, c, s, r);
    if (op.io.x & 1) {
        op_c(lay, c, ip, s, r, op.cf2, op.io.w);
        project(s, off);
    }
    store_state(lay, d, c, ip, w, s, off);
    count_next_graph(lay, d, w, s.s_pos, s.sdeg, s.b, s.nl, s.n, s.pb, s.qb);
    count_evaluation(lay, w, s);
}

// k_step_count on the loaded sample: one posterior step fused with pass 1 of the radius graph of the sample's next evaluation
template <class Eps, class MeanX>
__device__ __forceinline__ void plain_op(const Layout& lay, const Dims& d, const ChainBuf& c, const Work& w, const StepWg& s, const StepRows& r,
                                         Eps eps_of, MeanX mean_x) {
    op_a(lay, c, s, r, 1 + s.step, eps_of, mean_x);
    project_store_plain(lay, d, c, w, s, r);
    count_next_graph(lay, d, w, s.s_pos, s.sdeg, s.b, s.nl, s.n, s.pb, s.qb);
    count_evaluation(lay, w, s);
}
