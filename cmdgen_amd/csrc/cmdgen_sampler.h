// cmdgen_sampler.h - device helpers of the conditional sampler kernels (kernels_ddpm.hip, kernels_score.hip, and through cmdgen_step_parts.h, which
// composes the derived chains' step kernels from them, kernels_inpaint.hip, kernels_multi.hip and kernels_restrain.hip).
// These translation units are built with -ffp-contract=off, so the same helper rounds the same way in each.
#pragma once
#include "cmdgen_dev.h"
#include "cmdgen_launch.h"

__device__ __forceinline__ void atomic_max_pos(unsigned int* slot, float v) {
    atomicMax(slot, __float_as_uint(fabsf(v)) & 0x7fffffffu);     // non-negative floats order like their bits (a NaN's sign bit is cleared: any NaN ranks above +Inf)
}

// max that keeps a NaN (fmaxf drops it): torch's x.abs().max() returns NaN as soon as one element is NaN, and the
// reference's assertion then fails (NaN < 1e-2 is False) - so a NaN must survive into the recorded maxima
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? __uint_as_float(0x7fc00000u) : fmaxf(a, b); }

// records the two maxima assert_mean_zero_with_mask compares (en_diffusion.py:919-924).  Non-negative floats order like
// their bits and the quiet NaN 0x7fc00000 lies above +Inf, so atomicMax on the bits keeps a NaN once one sample has it.
__device__ __forceinline__ void record_com_check(unsigned int* slot2, const float* zx, int ld, int pb,
                                                 int nl, float scale, int lane) {
    float mx = 0.f;
    for (int i = lane; i < nl; i += 64) {
        const float* p = zx + (size_t)(pb + i) * ld;
        mx = max_nan(mx, max_nan(fabsf(p[0] * scale), max_nan(fabsf(p[1] * scale), fabsf(p[2] * scale))));
    }
    for (int o = 32; o > 0; o >>= 1) mx = max_nan(mx, __shfl_xor(mx, o));
    float s = 0.f;
    if (lane < 3) for (int i = 0; i < nl; ++i) s += zx[(size_t)(pb + i) * ld + lane] * scale;
    s = fabsf(s);
    s = max_nan(s, max_nan(__shfl(s, 1), __shfl(s, 2)));
    if (lane == 0) { atomic_max_pos(slot2, mx); atomic_max_pos(slot2 + 1, s); }
}

// One draw of a derived chain, component comp of row `local` of sample b's rows: injected noise row `row` ([stride] rows per draw, the sample's first
// at `base`: Layout::Nl and phar_base[b], or for a group GroupTab::Nu and ubase[b]), or Philox keyed by Layout::pocket_gid[b] (the sample's global
// pocket id, or its group's id, which every member holds) with the draw counter `key`.  Row and counter are given apart: the edit plan's rows are in
// call order, its counters are not.
__device__ __forceinline__ float chain_draw(const ChainBuf& c, const Layout& lay, int stride, int base, int row, int key, int b, int local, int comp,
                                            int ld) {
    if (c.noise) return c.noise[((size_t)row * stride + base + local) * ld + comp];
    float z[4];
    philox_normal4(c.seed, (uint32_t)lay.pocket_gid[b], (uint32_t)(lay.pocket_gid[b] >> 32),
                   (uint32_t)key, (uint32_t)(local * 4 + (comp >> 2)), z);
    return z[comp & 3];
}

// ---- groups of samples that share one latent (kernels_multi.hip, and the multi-pocket scoring chain of kernels_score.hip)
// one draw per group and op: chain_draw(c, lay, g.Nu, g.ubase[b], draw_idx, draw_idx, ...), written out because the multi-pocket scoring kernels
// (kernels_score.hip) call it and are scheduled differently through the forwarding call
__device__ __forceinline__ float draw_group(const ChainBuf& c, const Layout& lay, const GroupTab& g, int draw_idx, int b,
                                            int local, int comp, int ld) {
    if (c.noise) return c.noise[((size_t)draw_idx * g.Nu + g.ubase[b] + local) * ld + comp];
    float z[4];
    philox_normal4(c.seed, (uint32_t)lay.pocket_gid[b], (uint32_t)(lay.pocket_gid[b] >> 32),
                   (uint32_t)draw_idx, (uint32_t)(local * 4 + (comp >> 2)), z);
    return z[comp & 3];
}

// eps_bar of element idx of the group's rows (eps: [Nl][ld], a member's rows start at its phar_base)
__device__ __forceinline__ float combine_eps(const Layout& lay, const GroupTab& g, const float* __restrict__ eps, int first, int M,
                                             int ld, int idx) {
    float e = g.weight[first] * eps[(size_t)lay.phar_base[first] * ld + idx];
    for (int m = 1; m < M; ++m) e = e + g.weight[first + m] * eps[(size_t)lay.phar_base[first + m] * ld + idx];
    return e;
}

// ---- parts of the kernels that hold a sample's z and positions in LDS (cmdgen_step_parts.h, k_multi_score_step)
// the phar centre of mass of the sample's z (LDS, index order, as index_add_) on threads 0..2 -> s_mean
__device__ __forceinline__ void phar_mean(const float* s_z, int nl, int ld, int tid, float* s_mean) {
    if (tid < 3) {
        float sum = 0.f;
        for (int i = 0; i < nl; ++i) sum += s_z[i * ld + tid];
        s_mean[tid] = sum / fmaxf((float)nl, 1.0f);
    }
}

// subtract (m0, m1, m2) from the phar x columns in LDS and from the pocket positions in LDS (rows nl .. n-1 of s_pos)
__device__ __forceinline__ void sub_mean(float* s_z, float4* s_pos, int nl, int n, int ld, int tid, int nt, float m0, float m1, float m2) {
    for (int i = tid; i < n; i += nt) {
        if (i < nl) { float* z = s_z + i * ld; z[0] -= m0; z[1] -= m1; z[2] -= m2; }
        else { float4 p = s_pos[i]; p.x -= m0; p.y -= m1; p.z -= m2; s_pos[i] = p; }
    }
}

// pass 1 of the radius graph of the NEXT evaluation from the sample's final positions in LDS (s_pos[0 .. n-1], phar rows first), as
// k_edge_count and the tail of k_step_count: a row per wave, the degrees in sdeg and degL, the sample's four edge totals.  The whole
// workgroup calls it after a barrier that follows the last write to s_pos.
__device__ __forceinline__ void count_next_graph(const Layout& lay, const Dims& d, const Work& w, const float4* s_pos, int* sdeg, int b,
                                                 int nl, int n, int pb, int qb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
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
}
