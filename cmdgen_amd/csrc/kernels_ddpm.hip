// kernels_ddpm.hip - the ancestral-sampling arithmetic around the network evaluation:
// ConditionalDDPM.sample_given_pocket (conditional_model.py:388-465).  One wave per sample;
// sums that the reference forms with scatter_add/scatter_mean in index order are formed in
// the same order here (a lane walks the sample's nodes) so results agree to the last bit
// given the same inputs.
#include "cmdgen_sampler.h"

__device__ __forceinline__ float draw(const ChainBuf& c, const Layout& lay, int draw_idx, int b,
                                      int local, int node, int comp, int ld) {
    if (c.noise) return c.noise[((size_t)draw_idx * lay.Nl + node) * ld + comp];
    float z[4];
    philox_normal4(c.seed, (uint32_t)lay.pocket_gid[b], (uint32_t)(lay.pocket_gid[b] >> 32),
                   (uint32_t)draw_idx, (uint32_t)(local * 4 + (comp >> 2)), z);
    return z[comp & 3];
}

// subtract the phar centre of mass from phar and pocket coordinates of sample b
// (remove_mean_batch, conditional_model.py:467-475); returns nothing, works in place.
__device__ __forceinline__ void remove_com(float* zx, int ld, int pb, int nl, float* px, int ldq,
                                           int qb, int np, int lane) {
    float mean = 0.f;
    if (lane < 3) {
        float s = 0.f;
        for (int i = 0; i < nl; ++i) s += zx[(size_t)(pb + i) * ld + lane];   // index order, as index_add_
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

// z_T = [pocket COM, 0] + noise, then COM projection (conditional_model.py:402-420)
__global__ __launch_bounds__(64) void k_chain_init(Layout lay, Dims d, ChainBuf c,
                                                   const float* __restrict__ pocket_x,
                                                   const float* __restrict__ pocket_onehot) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b];
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    // normalize (en_diffusion.py:874-889)
    for (int i = lane; i < np; i += 64) {
        float* o = c.xh_pocket + (size_t)(qb + i) * ldq;
        for (int k = 0; k < 3; ++k) o[k] = pocket_x[(size_t)(qb + i) * 3 + k] / d.norm_x;
        for (int k = 0; k < d.R; ++k) o[3 + k] = (pocket_onehot[(size_t)(qb + i) * d.R + k] - d.bias_h) / d.norm_h;
    }
    __syncthreads();
    if (d.no_com) {      // SimpleConditionalDDPM.sample_given_pocket :512-521: subtract the pocket COM once (un-normalised x; norm_x divides both)
        float pm = 0.f;
        if (lane < 3) {
            float s = 0.f;
            for (int i = 0; i < np; ++i) s += pocket_x[(size_t)(qb + i) * 3 + lane];
            pm = s / fmaxf((float)np, 1.0f);
        }
        const float p0 = __shfl(pm, 0), p1 = __shfl(pm, 1), p2 = __shfl(pm, 2);
        for (int i = lane; i < np; i += 64) {
            float* o = c.xh_pocket + (size_t)(qb + i) * ldq;
            o[0] = (pocket_x[(size_t)(qb + i) * 3 + 0] - p0) / d.norm_x;
            o[1] = (pocket_x[(size_t)(qb + i) * 3 + 1] - p1) / d.norm_x;
            o[2] = (pocket_x[(size_t)(qb + i) * 3 + 2] - p2) / d.norm_x;
        }
        __syncthreads();
    }
    float mu = 0.f;
    if (lane < 3) {
        float s = 0.f;
        for (int i = 0; i < np; ++i) s += c.xh_pocket[(size_t)(qb + i) * ldq + lane];
        mu = s / fmaxf((float)np, 1.0f);
    }
    const float m0 = __shfl(mu, 0), m1 = __shfl(mu, 1), m2 = __shfl(mu, 2);
    for (int idx = lane; idx < nl * ld; idx += 64) {
        const int i = idx / ld, k = idx % ld;
        const float m = k == 0 ? m0 : k == 1 ? m1 : k == 2 ? m2 : 0.f;
        c.z_phar[(size_t)(pb + i) * ld + k] = m + 1.0f * draw(c, lay, 0, b, i, pb + i, k, ld);
    }
    __syncthreads();
    if (d.no_com) return;                       // no projection, and the mean-zero assertion is a no-op (:503-505)
    remove_com(c.z_phar, ld, pb, nl, c.xh_pocket, ldq, qb, np, lane);
    __syncthreads();
    record_com_check(c.check, c.z_phar, ld, pb, nl, 1.0f, lane);
}

// p(x, h | z_0): sample_p_xh_given_z0 (conditional_model.py:108-131) + unnormalize + one-hot
__global__ __launch_bounds__(64) void k_chain_final(Layout lay, Dims d, ChainBuf c, Work w,
                                                    const float* __restrict__ eps,
                                                    float* __restrict__ xh_phar_out,
                                                    float* __restrict__ xh_pocket_out,
                                                    unsigned int* cog_slot) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b];
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    const int K = c.state->K;
    const float4 cf = c.coef[K];                    // (sigma_0, alpha_0, sigma_x = exp(gamma_0/2), 0)
    const bool nan_reset = *w.nan_flag != 0;
    // types come from z_0 itself (not from the sampled xh): argmax of the un-normalised h
    for (int i = lane; i < nl; i += 64) {
        const float* z = c.z_phar + (size_t)(pb + i) * ld;
        int best = 0; float bv = z[3] * d.norm_h + d.bias_h;
        for (int k = 1; k < d.P; ++k) { const float v = z[3 + k] * d.norm_h + d.bias_h; if (v > bv) { bv = v; best = k; } }
        float* o = xh_phar_out + (size_t)(pb + i) * ld;
        for (int k = 0; k < d.P; ++k) o[3 + k] = (k == best) ? 1.0f : 0.0f;
    }
    __syncthreads();
    // mu_x = 1/alpha_0 * (z_0 - sigma_0 * eps)  (compute_x_pred, en_diffusion.py:153-165); + sigma_x * noise
    for (int idx = lane; idx < nl * ld; idx += 64) {
        const int i = idx / ld, k = idx % ld;
        const size_t o = (size_t)(pb + i) * ld + k;
        float e = eps[o];
        if (nan_reset && k < 3) e = 0.f;
        const float mu = (1.0f / cf.y) * (c.z_phar[o] - cf.x * e);
        c.z_phar[o] = mu + cf.z * draw(c, lay, 1 + K, b, i, pb + i, k, ld);
    }
    __syncthreads();
    if (!d.no_com) remove_com(c.z_phar, ld, pb, nl, c.xh_pocket, ldq, qb, np, lane);
    __syncthreads();
    // unnormalize (en_diffusion.py:891-895)
    for (int i = lane; i < nl; i += 64) {
        const float* z = c.z_phar + (size_t)(pb + i) * ld;
        float* o = xh_phar_out + (size_t)(pb + i) * ld;
        o[0] = z[0] * d.norm_x; o[1] = z[1] * d.norm_x; o[2] = z[2] * d.norm_x;
    }
    for (int i = lane; i < np; i += 64) {
        const float* q = c.xh_pocket + (size_t)(qb + i) * ldq;
        float* o = xh_pocket_out + (size_t)(qb + i) * ldq;
        o[0] = q[0] * d.norm_x; o[1] = q[1] * d.norm_x; o[2] = q[2] * d.norm_x;
        for (int k = 0; k < d.R; ++k) o[3 + k] = q[3 + k] * d.norm_h + d.bias_h;
    }
    __syncthreads();
    if (!d.no_com) record_com_check(c.check + 2 * (1 + K), xh_phar_out, ld, pb, nl, 1.0f, lane);
    // CoG drift of the un-normalised coordinates (conditional_model.py:451-452)
    float s = 0.f;
    if (lane < 3) for (int i = 0; i < nl; ++i) s += xh_phar_out[(size_t)(pb + i) * ld + lane];
    s = fabsf(s);
    s = max_nan(s, max_nan(__shfl(s, 1), __shfl(s, 2)));
    if (lane == 0) atomic_max_pos(cog_slot, s);
    if (b == 0 && lane == 0 && nan_reset) atomicAdd(&w.counters[4], 1ull);
}

// if the batch-wide max drift exceeds 5e-2 every sample is re-centred (conditional_model.py:453-457)
__global__ __launch_bounds__(64) void k_chain_drift_fix(Layout lay, Dims d, float* __restrict__ xh_phar_out,
                                                        float* __restrict__ xh_pocket_out,
                                                        const unsigned int* cog_slot) {
    if (d.no_com || !(__uint_as_float(*cog_slot) > 5e-2f)) return;       // the simple variant's re-centring is the identity (:500-501)
    const int b = blockIdx.x, lane = threadIdx.x;
    remove_com(xh_phar_out, 3 + d.P, lay.phar_base[b], lay.num_phar[b], xh_pocket_out, 3 + d.R,
               lay.pocket_base[b], lay.num_pocket[b], lane);
}

// ------------------------------------------------------------------------------------------------------------
// k_step_count: one posterior step z_t -> z_s (sample_p_zs_given_zt, conditional_model.py:342-374) FUSED with pass 1
// of the next evaluation's radius graph (k_edge_count, kernels_egnn.hip): both are one-workgroup-per-sample, and the
// new positions are already in LDS when the step is done - one launch and one global round trip of the positions less
// per denoising step.  256 threads per sample.  The sample's z is pulled into LDS with all loads in flight; the sums of
// the step (COM check, centre of mass) walk LDS in node index order; the count pass is k_edge_count's (same dist2,
// same ballots).
// own_vel (readout_mode, cmdgen_dev.h: the evaluation ran without k_readout): nobody wrote the velocity columns of eps or the NaN flag.  The
// workgroup forms the velocities of its sample's rows itself (readout_vel), and - the flag is batch-global (dynamics.py:129-131) - evaluates
// the same expression for ALL Nl phar rows and ORs isnan over the workgroup: every workgroup reaches the same flag on its own, none learns
// anything from another.  So nothing the scan reads (X0, XL, ACC, adiv) may change during this launch: X0 and ACC are left to pass 2 of the
// radius graph (edge_write_body), the launch behind this one.
// ------------------------------------------------------------------------------------------------------------
// (a template parameter: the form without it stays the code it was)
template <bool own_vel>
__global__ __launch_bounds__(1024) void k_step_count(Layout lay, Dims d, ChainBuf c, Work w,
                                                    const float* __restrict__ eps) {
    extern __shared__ float4 s_pos[];               // [max_n] positions of the sample (phar first), then int sdeg[max_n], then z
    int* sdeg = reinterpret_cast<int*>(s_pos + lay.max_n);
    float* s_z = reinterpret_cast<float*>(sdeg + lay.max_n);      // [nl * ld]
    float* s_vel = s_z + (size_t)lay.max_n * (3 + d.P);           // own_vel: [nl][3]
    __shared__ float s_mean[3];
    __shared__ int s_bad[16];                                      // own_vel: per wave, did a lane see a NaN velocity?
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int nl = lay.num_phar[b], np = lay.num_pocket[b], n = nl + np;
    const int pb = lay.phar_base[b], qb = lay.pocket_base[b];
    const int ld = 3 + d.P, ldq = 3 + d.R;
    const int step = c.state->step - 1;
    const float4 cf = c.coef[step];
    float* zg = c.z_phar + (size_t)pb * ld;
    const float* eg = eps + (size_t)pb * ld;
    const int cnt = nl * ld;
    const int flag0 = own_vel ? 0 : *w.nan_flag;                  // (requested with the kernel's first scalar loads, as before)
    // own_vel: the operands of the first four rows of this thread's share of the scan are requested here, in front of the kernel's first loads, and
    // used behind them - one round trip for all of them (at 64 pockets of 15 points: the whole scan; the compiled kernel issues its 12 global_load_dwordx3
    // - the w components are never used - back to back in front of the first s_waitcnt: 56 registers)
    [[maybe_unused]] VelIn vin[4];
    if constexpr (own_vel) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = tid + u * (int)blockDim.x;
            if (r < lay.Nl) vin[u] = readout_vel_in(lay, w, d, r);
        }
    }
    for (int idx = tid; idx < cnt; idx += blockDim.x) s_z[idx] = zg[idx];
    // pocket coordinates of this sample: in flight while the step is computed
    for (int i = tid; i < np; i += blockDim.x) {
        const float* q = c.xh_pocket + (size_t)(qb + i) * ldq;
        s_pos[nl + i] = make_float4(q[0], q[1], q[2], 0.f);
    }
    if constexpr (own_vel) {
        int bad = 0;
        auto take = [&](int r, const float4& v) {
            bad |= vel_isnan(v) ? 1 : 0;
            const int i = r - pb;
            if (i >= 0 && i < nl) { s_vel[3 * i] = v.x; s_vel[3 * i + 1] = v.y; s_vel[3 * i + 2] = v.z; }
        };
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = tid + u * (int)blockDim.x;
            if (r < lay.Nl) take(r, readout_vel_of(vin[u]));
        }
        for (int r = tid + 4 * (int)blockDim.x; r < lay.Nl; r += (int)blockDim.x) take(r, readout_vel(lay, w, d, r));     // (more than 4 rows per thread)
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
    if (wave == 0 && !d.no_com) record_com_check(c.check + 2 * (1 + step), s_z, ld, 0, nl, 1.0f, lane);   // z_t, the step's input
    __syncthreads();
    for (int idx = tid; idx < cnt; idx += blockDim.x) {
        const int i = idx / ld, k = idx - i * ld;
        float e = eg[idx];                          // (unconditional, so it is requested ahead of the barriers as before; own_vel: columns 0..2 are stale and unused)
        if constexpr (own_vel) { if (k < 3) e = s_vel[3 * i + k]; }
        if (nan_reset && k < 3) e = 0.f;
        const float mu = s_z[idx] / cf.x - cf.y * e;
        s_z[idx] = mu + cf.z * draw(c, lay, 1 + step, b, i, pb + i, k, ld);
    }
    __syncthreads();
    if (tid < 3) {                                  // phar centre of mass, index order (remove_mean_batch :467-475)
        float sum = 0.f;
        if (!d.no_com) {
            for (int i = 0; i < nl; ++i) sum += s_z[i * ld + tid];
            sum = sum / fmaxf((float)nl, 1.0f);
        }
        s_mean[tid] = sum;
    }
    __syncthreads();
    const float m0 = s_mean[0], m1 = s_mean[1], m2 = s_mean[2];
    for (int i = tid; i < n; i += blockDim.x) {
        float4 p;
        if (i < nl) {
            float* z = s_z + i * ld;
            if (!d.no_com) { z[0] -= m0; z[1] -= m1; z[2] -= m2; }
            p = make_float4(z[0], z[1], z[2], 0.f);
            if constexpr (!own_vel) {         // (own_vel: other workgroups are reading both - pass 2 stores them from z_phar)
                w.X0[pb + i] = p;
                for (int l = 0; l < d.L; ++l) w.ACC[(size_t)l * lay.Nm + pb + i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            p = s_pos[i];
            if (!d.no_com) {
                p.x -= m0; p.y -= m1; p.z -= m2;
                float* q = c.xh_pocket + (size_t)(qb + i - nl) * ldq;
                q[0] = p.x; q[1] = p.y; q[2] = p.z;
            }
            w.XP[qb + i - nl] = p;
            if (c.pocket_steps) {
                float* o = c.pocket_steps + ((size_t)step * lay.Np + qb + i - nl) * 3;
                o[0] = p.x; o[1] = p.y; o[2] = p.z;
            }
        }
        s_pos[i] = p;
    }
    __syncthreads();
    for (int idx = tid; idx < cnt; idx += blockDim.x) {
        const float v = s_z[idx];
        zg[idx] = v;
        if (c.z_steps) c.z_steps[(size_t)step * lay.Nl * ld + (size_t)pb * ld + idx] = v;
    }
    // ---- pass 1 of the radius graph of the NEXT evaluation (as k_edge_count)
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

// (The NaN flag this kernel reads is cleared for the next evaluation by k_edge_write, which runs after every reader
// of the old value and before k_readout - or k_vel_flag in front of the decode - can set it again.)

void cmdgen_launch_chain_init(const Layout& lay, const Dims& d, const ChainBuf& c, const float* px,
                              const float* poh, hipStream_t s) {
    hipLaunchKernelGGL(k_chain_init, dim3(lay.B), dim3(64), 0, s, lay, d, c, px, poh);
}
void cmdgen_launch_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const Work& w,
                              const float* eps, int own_vel, hipStream_t s) {
    const size_t shm = (size_t)lay.max_n * (sizeof(float4) + sizeof(int)) + (size_t)lay.max_n * (3 + d.P + (own_vel ? 3 : 0)) * sizeof(float);
    if (own_vel) hipLaunchKernelGGL(k_step_count<true>, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), shm, s, lay, d, c, w, eps);
    else hipLaunchKernelGGL(k_step_count<false>, dim3(lay.B), dim3(lay.max_n > 128 ? 1024 : 256), shm, s, lay, d, c, w, eps);     // 16 waves for big samples (one receiver per wave at a time)
}
void cmdgen_launch_chain_final(const Layout& lay, const Dims& d, const ChainBuf& c, const Work& w,
                               const float* eps, float* xo, float* po, unsigned int* cog, hipStream_t s) {
    hipLaunchKernelGGL(k_chain_final, dim3(lay.B), dim3(64), 0, s, lay, d, c, w, eps, xo, po, cog);
    hipLaunchKernelGGL(k_chain_drift_fix, dim3(lay.B), dim3(64), 0, s, lay, d, xo, po, (const unsigned int*)cog);
}

// same generator as draw() above, exposed for statistical tests
__global__ void k_debug_noise(unsigned long long seed, long long pocket_id, int draw_idx, int n_nodes, int width,
                              float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_nodes * width) return;
    const int local = idx / width, comp = idx - local * width;
    float z[4];
    philox_normal4(seed, (uint32_t)pocket_id, (uint32_t)((unsigned long long)pocket_id >> 32), (uint32_t)draw_idx,
                   (uint32_t)(local * 4 + (comp >> 2)), z);
    out[idx] = z[comp & 3];
}
void cmdgen_launch_debug_noise(unsigned long long seed, long long pocket_id, int draw, int n_nodes, int width,
                               float* out, hipStream_t s) {
    const int n = n_nodes * width;
    hipLaunchKernelGGL(k_debug_noise, dim3((n + 255) / 256), dim3(256), 0, s, seed, pocket_id, draw, n_nodes, width, out);
}
