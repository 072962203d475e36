// kernels_train_loss.hip - the loss side of the training step (noising, the per-sample loss terms with dL/d eps, their batch means) for the
// conditional, simple and joint models, AdamW with the gradient norm, and the half engine's range guards; each with its launcher.
// (k_train_loss keeps its own copy of the per-part body and of log p(h | z_0) that k_train_loss_joint has as pieces: DESIGN.md 6c.)
#include "cmdgen_train_parts.h"

// ------------------------------------------------------------------------------------
// The loss side of the conditional training step (conditional_model.py:198-320 + lightning_modules.py:188-239 of the
// reference) as three launches instead of ~270 small tensor ops: the noising of a batch (normalize, remove_mean_batch,
// noised_representation), the per-sample loss terms together with dL/d eps, and their batch means.  One workgroup per
// sample (a sample has tens of phar nodes and tens to hundreds of pocket nodes); the per-sample scalars that depend
// only on t and on the node counts (alpha_t, sigma_t, SNR weight, the normalisation constants, log p(N)) come from the
// host in `tab`, column-major [TT_COLS][B].
// ------------------------------------------------------------------------------------
enum { TT_ALPHA_T = 0, TT_SIGMA_T, TT_T0, TT_SNRW, TT_ALPHA_TT, TT_SIGMA_TT, TT_NEGLOGC, TT_DLOGPX, TT_LOGPN, TT_TINT, TT_T, TT_S0CAT, TT_COLS };
enum { TS_NLL = 0, TS_ERR_T, TS_LOSS_0, TS_KL, TS_ABS_X, TS_ABS_H, TS_LOSS_0X, TS_LOSS_0H, TS_LOSS_T, TS_COLS = 12 };

// sum of up to three per-thread values over a 256-thread workgroup; every thread gets the totals
__device__ __forceinline__ void wg_sum3(float& a, float& b, float& c, float* red /* [12] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); c += __shfl_xor(c, o); }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[4 + w] = b; red[8 + w] = c; }
    __syncthreads();
    a = (red[0] + red[1]) + (red[2] + red[3]); b = (red[4] + red[5]) + (red[6] + red[7]); c = (red[8] + red[9]) + (red[10] + red[11]);
}

// z_t, the centred pocket and the two sums of the prior KL term of every sample
__global__ __launch_bounds__(256) void k_train_noise(Layout lay, Dims d, const float* __restrict__ px, const float* __restrict__ poh,
                                                     const float* __restrict__ qx, const float* __restrict__ qoh,
                                                     const float* __restrict__ tab, const float* __restrict__ eps,
                                                     float* __restrict__ z_t, float* __restrict__ xh_pocket, float* __restrict__ klsum) {
    __shared__ float red[12];
    const int b = blockIdx.x, B = lay.B, tid = threadIdx.x;
    const int n = lay.num_phar[b], base = lay.phar_base[b], m = lay.num_pocket[b], qbase = lay.pocket_base[b];
    const int P = d.P, R = d.R, ldp = 3 + P, ldq = 3 + R;
    const float alpha = tab[TT_ALPHA_T * B + b], sigma = tab[TT_SIGMA_T * B + b], alphaT = tab[TT_ALPHA_TT * B + b];
    const float cnt = (float)max(n, 1);
    // phar centre of mass of the normalised coordinates (remove_mean_batch #1); SimpleConditionalDDPM (d.no_com): the POCKET's centre
    // of mass of the raw coordinates, subtracted before normalisation (conditional_model.py:481-525), and no projection afterwards
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if (d.no_com) {
        for (int i = tid; i < m; i += 256) { const float* x = qx + (size_t)(qbase + i) * 3; sx += x[0]; sy += x[1]; sz += x[2]; }
    } else {
        for (int i = tid; i < n; i += 256) {
            const float* x = px + (size_t)(base + i) * 3;
            sx += x[0] / d.norm_x; sy += x[1] / d.norm_x; sz += x[2] / d.norm_x;
        }
    }
    wg_sum3(sx, sy, sz, red);
    const float cq = (float)max(m, 1);
    const float m1x = d.no_com ? sx / cq : sx / cnt, m1y = d.no_com ? sy / cq : sy / cnt, m1z = d.no_com ? sz / cq : sz / cnt;
    // (conditional: m1 is in normalised units and subtracted after the division; simple: raw units, subtracted before it)
#define TN_X(v, mm) (d.no_com ? ((v) - (mm)) / d.norm_x : (v) / d.norm_x - (mm))
    // z_t = alpha xh0 + sigma eps (x part still with its mean), the KL sums of alpha_T xh0
    float zx = 0.f, zy = 0.f, zz = 0.f, klx = 0.f, klh = 0.f, dummy = 0.f;
    for (int i = tid; i < n; i += 256) {
        const size_t g = (size_t)(base + i);
        const float* x = px + g * 3; const float* e = eps + g * ldp; float* z = z_t + g * ldp;
        const float x0 = TN_X(x[0], m1x), x1 = TN_X(x[1], m1y), x2 = TN_X(x[2], m1z);
        const float a0 = alphaT * x0, a1 = alphaT * x1, a2 = alphaT * x2;
        klx += a0 * a0 + a1 * a1 + a2 * a2;
        const float z0 = alpha * x0 + sigma * e[0], z1 = alpha * x1 + sigma * e[1], z2 = alpha * x2 + sigma * e[2];
        z[0] = z0; z[1] = z1; z[2] = z2; zx += z0; zy += z1; zz += z2;
        for (int c = 0; c < P; ++c) {
            const float h = (poh[g * P + c] - d.bias_h) / d.norm_h, ah = alphaT * h;
            klh += ah * ah;
            z[3 + c] = alpha * h + sigma * e[3 + c];
        }
    }
    wg_sum3(zx, zy, zz, red);
    wg_sum3(klx, klh, dummy, red);
    const float m2x = d.no_com ? 0.f : zx / cnt, m2y = d.no_com ? 0.f : zy / cnt, m2z = d.no_com ? 0.f : zz / cnt;
    if (!d.no_com)
        for (int i = tid; i < n; i += 256) {        // remove_mean_batch #2 (each thread revisits the rows it wrote)
            float* z = z_t + (size_t)(base + i) * ldp;
            z[0] -= m2x; z[1] -= m2y; z[2] -= m2z;
        }
    for (int i = tid; i < m; i += 256) {
        const size_t g = (size_t)(qbase + i);
        const float* x = qx + g * 3; float* o = xh_pocket + g * ldq;
        o[0] = TN_X(x[0], m1x) - m2x; o[1] = TN_X(x[1], m1y) - m2y; o[2] = TN_X(x[2], m1z) - m2z;
        for (int c = 0; c < R; ++c) o[3 + c] = (qoh[g * R + c] - d.bias_h) / d.norm_h;
    }
    if (tid == 0) { klsum[2 * b] = klx; klsum[2 * b + 1] = klh; }
#undef TN_X
}

__device__ __forceinline__ float cdf_std_gauss(float x) { return 0.5f * (1.0f + erff(x / 1.41421356237309515f)); }

// per-sample loss terms and dL/d net_out.  l2: the 'l2' training objective (lightning_modules.py:198-205), else the vlb
// weighting (:206-212); both in training mode (t = 0 handled by the t_is_zero masks, conditional_model.py:265-272).
__global__ __launch_bounds__(256) void k_train_loss(Layout lay, Dims d, int l2, float T, const float* __restrict__ net,
                                                    const float* __restrict__ eps, const float* __restrict__ z_t,
                                                    const float* __restrict__ poh, const float* __restrict__ tab,
                                                    const float* __restrict__ klsum, float* __restrict__ terms,
                                                    float* __restrict__ d_eps) {
    __shared__ float red[12];
    const int b = blockIdx.x, B = lay.B, tid = threadIdx.x;
    const int n = lay.num_phar[b], base = lay.phar_base[b];
    const int P = d.P, ldp = 3 + P;
    const float t0 = tab[TT_T0 * B + b], snrw = tab[TT_SNRW * B + b], s0cat = tab[TT_S0CAT * B + b];
    const float nf = (float)n;
    const float s_t = l2 ? 1.0f / ((float)(3 + P) * nf) : -T * snrw, s_0 = l2 ? 1.0f / (3.0f * nf) : 1.0f;
    const float w_t = (1.0f - t0) * s_t / (float)B, w_0 = t0 * s_0 / (float)B;
    float ex = 0.f, eh = 0.f, lph = 0.f, ax = 0.f, ah = 0.f, dummy = 0.f;
    for (int i = tid; i < n; i += 256) {
        const size_t g = (size_t)(base + i);
        const float* o = net + g * ldp; const float* e = eps + g * ldp; float* de = d_eps + g * ldp;
        float sabs = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float df = o[c] - e[c];
            ex += df * df; sabs += fabsf(o[c]);
            de[c] = df * w_t + df * w_0;
        }
        ax += sabs / 3.0f;
        sabs = 0.f;
        for (int c = 0; c < P; ++c) {
            const float df = o[3 + c] - e[3 + c];
            eh += df * df; sabs += fabsf(o[3 + c]);
            de[3 + c] = df * w_t;
        }
        ah += sabs / (float)P;
        // log p(h | z_0): integrate the normal around each class over the unit bin, normalise over the classes
        const float* z = z_t + g * ldp + 3;
        float mx = -INFINITY;
        for (int c = 0; c < P; ++c) {
            const float ctr = z[c] * d.norm_h + d.bias_h - 1.0f;
            const float lp = logf(cdf_std_gauss((ctr + 0.5f) / s0cat) - cdf_std_gauss((ctr - 0.5f) / s0cat) + 1e-10f);
            mx = fmaxf(mx, lp);
        }
        float se = 0.f, dot = 0.f, ohs = 0.f;
        for (int c = 0; c < P; ++c) {
            const float ctr = z[c] * d.norm_h + d.bias_h - 1.0f;
            const float lp = logf(cdf_std_gauss((ctr + 0.5f) / s0cat) - cdf_std_gauss((ctr - 0.5f) / s0cat) + 1e-10f);
            se += expf(lp - mx);
            const float oh = ((poh[g * P + c] - d.bias_h) / d.norm_h) * d.norm_h + d.bias_h;
            dot += lp * oh; ohs += oh;
        }
        lph += dot - (mx + logf(se)) * ohs;
    }
    wg_sum3(ex, eh, lph, red);
    wg_sum3(ax, ah, dummy, red);
    if (tid == 0) {
        const float alphaT = tab[TT_ALPHA_TT * B + b], sigT = tab[TT_SIGMA_TT * B + b];
        (void)alphaT;
        const float dsub = (d.no_com ? nf : nf - 1.0f) * 3.0f;      // subspace_dimensionality (SimpleConditionalDDPM: no projection)
        // gaussian_KL(|mu|^2, sigma_T, 1, dim) = dim log(1 / sigma_T) + 0.5 (dim sigma_T^2 + |mu|^2) - 0.5 dim
        const float kl_h = logf(1.0f / sigT) + 0.5f * (sigT * sigT + klsum[2 * b + 1]) - 0.5f;
        const float kl_x = dsub * logf(1.0f / sigT) + 0.5f * (dsub * sigT * sigT + klsum[2 * b]) / 1.0f - 0.5f * dsub;
        const float kl = kl_x + kl_h;
        float err_t = (ex + eh) * (1.0f - t0);
        const float loss_0x = 0.5f * ex * t0, loss_0h = -lph * t0;
        float loss_t, loss_0, nll;
        if (l2) {
            err_t = err_t / ((float)(3 + P) * nf);
            loss_t = 0.5f * err_t;
            loss_0 = loss_0x / (3.0f * nf) + loss_0h;
            nll = loss_t + loss_0 + kl;
        } else {
            loss_t = -T * 0.5f * snrw * err_t;
            loss_0 = loss_0x + loss_0h + tab[TT_NEGLOGC * B + b];
            nll = loss_t + loss_0 + kl - tab[TT_DLOGPX * B + b] - tab[TT_LOGPN * B + b];
        }
        const float cnt = (float)max(n, 1);
        float* o = terms + (size_t)b * TS_COLS;
        o[TS_NLL] = nll; o[TS_ERR_T] = err_t; o[TS_LOSS_0] = loss_0; o[TS_KL] = kl; o[TS_ABS_X] = ax / cnt; o[TS_ABS_H] = ah / cnt;
        o[TS_LOSS_0X] = loss_0x; o[TS_LOSS_0H] = loss_0h; o[TS_LOSS_T] = loss_t;
    }
}

// ------------------------------------------------------------------------------------
// The same two launches for the JOINT model (EnVariationalDiffusion.forward in training mode, en_diffusion.py:332-465, and the
// joint branch of lightning_modules.py:198-217): pocket nodes are noised and denoised too.  One workgroup per sample.
//   k_train_noise_joint: normalize; the x-part of the draw loses its centre of mass over ALL nodes of the sample
//     (sample_combined_position_feature_noise, :555-574); z = alpha_t xh + sigma_t eps for both parts; the prior-KL sums over both.
//   k_train_loss_joint: error_t, L0 (x of both parts, the categorical likelihood of both one-hot blocks), kl_prior with
//     (n_phar + n_pocket - 1) * 3 degrees of freedom, the 'l2' / vlb combination, dL/d net_out for both outputs.
// terms columns 0..8 as in k_train_loss (error_t / |eps_hat| of the phar part), 9 error_t of the pocket part, 10 / 11 mean
// |eps_hat| of the pocket's x / h.
// ------------------------------------------------------------------------------------
enum { TS_ERR_T_Q = 9, TS_ABS_X_Q = 10, TS_ABS_H_Q = 11 };

__global__ __launch_bounds__(256) void k_train_noise_joint(Layout lay, Dims d, const float* __restrict__ px, const float* __restrict__ poh,
                                                           const float* __restrict__ qx, const float* __restrict__ qoh,
                                                           const float* __restrict__ tab, const float* __restrict__ raw_l,
                                                           const float* __restrict__ raw_q, float* __restrict__ z_l, float* __restrict__ z_q,
                                                           float* __restrict__ e_l, float* __restrict__ e_q, float* __restrict__ klsum) {
    __shared__ float red[12];
    const int b = blockIdx.x, B = lay.B, tid = threadIdx.x;
    const int n = lay.num_phar[b], base = lay.phar_base[b], m = lay.num_pocket[b], qbase = lay.pocket_base[b];
    const int P = d.P, R = d.R, ldp = 3 + P, ldq = 3 + R;
    const float alpha = tab[TT_ALPHA_T * B + b], sigma = tab[TT_SIGMA_T * B + b], alphaT = tab[TT_ALPHA_TT * B + b];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = tid; i < n; i += 256) { const float* e = raw_l + (size_t)(base + i) * ldp; sx += e[0]; sy += e[1]; sz += e[2]; }
    for (int i = tid; i < m; i += 256) { const float* e = raw_q + (size_t)(qbase + i) * ldq; sx += e[0]; sy += e[1]; sz += e[2]; }
    wg_sum3(sx, sy, sz, red);
    const float cnt = (float)max(n + m, 1);
    const float mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
    float klx = 0.f, klh = 0.f, dummy = 0.f;
    auto part = [&](int rows, int row0, int C, int ld, const float* x3, const float* oh, const float* raw, float* z, float* eo) {
        for (int i = tid; i < rows; i += 256) {
            const size_t g = (size_t)(row0 + i);
            const float* x = x3 + g * 3; const float* e = raw + g * ld; float* zo = z + g * ld; float* ee = eo + g * ld;
            const float en[3] = {e[0] - mx, e[1] - my, e[2] - mz};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float xn = x[c] / d.norm_x, a = alphaT * xn;
                klx += a * a;
                ee[c] = en[c];
                zo[c] = alpha * xn + sigma * en[c];
            }
            for (int c = 0; c < C; ++c) {
                const float hn = (oh[g * C + c] - d.bias_h) / d.norm_h, a = alphaT * hn;
                klh += a * a;
                ee[3 + c] = e[3 + c];
                zo[3 + c] = alpha * hn + sigma * e[3 + c];
            }
        }
    };
    part(n, base, P, ldp, px, poh, raw_l, z_l, e_l);
    part(m, qbase, R, ldq, qx, qoh, raw_q, z_q, e_q);
    wg_sum3(klx, klh, dummy, red);
    if (tid == 0) { klsum[2 * b] = klx; klsum[2 * b + 1] = klh; }
}

// log p(h | z_0) of one node (en_diffusion.py:298-326): the normal around each class integrated over the unit bin, normalised over the
// classes, dotted with the node's one-hot row.  z: the node's normalised feature block; oh: its raw one-hot row.
__device__ __forceinline__ float log_ph_row(const float* z, const float* oh, int C, const Dims& d, float s0cat) {
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) {
        const float ctr = z[c] * d.norm_h + d.bias_h - 1.0f;
        mx = fmaxf(mx, logf(cdf_std_gauss((ctr + 0.5f) / s0cat) - cdf_std_gauss((ctr - 0.5f) / s0cat) + 1e-10f));
    }
    float se = 0.f, dot = 0.f, ohs = 0.f;
    for (int c = 0; c < C; ++c) {
        const float ctr = z[c] * d.norm_h + d.bias_h - 1.0f;
        const float lp = logf(cdf_std_gauss((ctr + 0.5f) / s0cat) - cdf_std_gauss((ctr - 0.5f) / s0cat) + 1e-10f);
        se += expf(lp - mx);
        const float o = ((oh[c] - d.bias_h) / d.norm_h) * d.norm_h + d.bias_h;
        dot += lp * o; ohs += o;
    }
    return dot - (mx + logf(se)) * ohs;
}

__global__ __launch_bounds__(256) void k_train_loss_joint(Layout lay, Dims d, int l2, float T, const float* __restrict__ net_l,
                                                          const float* __restrict__ net_q, const float* __restrict__ e_l,
                                                          const float* __restrict__ e_q, const float* __restrict__ z_l,
                                                          const float* __restrict__ z_q, const float* __restrict__ poh,
                                                          const float* __restrict__ qoh, const float* __restrict__ tab,
                                                          const float* __restrict__ klsum, float* __restrict__ terms,
                                                          float* __restrict__ d_l, float* __restrict__ d_q) {
    __shared__ float red[12];
    const int b = blockIdx.x, B = lay.B, tid = threadIdx.x;
    const int n = lay.num_phar[b], base = lay.phar_base[b], m = lay.num_pocket[b], qbase = lay.pocket_base[b];
    const int P = d.P, R = d.R;
    const float t0 = tab[TT_T0 * B + b], snrw = tab[TT_SNRW * B + b], s0cat = tab[TT_S0CAT * B + b];
    const float nf = (float)n, mf = (float)m;
    float sums[2][5];                      // [part][x error, h error, log p(h), |eps_hat_x|, |eps_hat_h|]
    auto part = [&](int which, int rows, int row0, int C, float cntf, const float* net, const float* eps, const float* z, const float* oh, float* de) {
        const int ld = 3 + C;
        const float s_t = l2 ? 1.0f / ((float)(3 + C) * cntf) : -T * snrw, s_0 = l2 ? 1.0f / (3.0f * cntf) : 1.0f;
        const float w_t = (1.0f - t0) * s_t / (float)B, w_0 = t0 * s_0 / (float)B;
        float ex = 0.f, eh = 0.f, lph = 0.f, ax = 0.f, ah = 0.f, dummy = 0.f;
        for (int i = tid; i < rows; i += 256) {
            const size_t g = (size_t)(row0 + i);
            const float* o = net + g * ld; const float* e = eps + g * ld; float* dd = de + g * ld;
            float sabs = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float df = o[c] - e[c];
                ex += df * df; sabs += fabsf(o[c]);
                dd[c] = df * w_t + df * w_0;
            }
            ax += sabs / 3.0f;
            sabs = 0.f;
            for (int c = 0; c < C; ++c) {
                const float df = o[3 + c] - e[3 + c];
                eh += df * df; sabs += fabsf(o[3 + c]);
                dd[3 + c] = df * w_t;
            }
            ah += sabs / (float)C;
            lph += log_ph_row(z + g * ld + 3, oh + g * C, C, d, s0cat);
        }
        wg_sum3(ex, eh, lph, red);
        wg_sum3(ax, ah, dummy, red);
        sums[which][0] = ex; sums[which][1] = eh; sums[which][2] = lph; sums[which][3] = ax; sums[which][4] = ah;
    };
    part(0, n, base, P, nf, net_l, e_l, z_l, poh, d_l);
    part(1, m, qbase, R, mf, net_q, e_q, z_q, qoh, d_q);
    if (tid == 0) {
        const float sigT = tab[TT_SIGMA_TT * B + b];
        const float dsub = (nf + mf - 1.0f) * 3.0f;
        const float kl_h = logf(1.0f / sigT) + 0.5f * (sigT * sigT + klsum[2 * b + 1]) - 0.5f;
        const float kl_x = dsub * logf(1.0f / sigT) + 0.5f * (dsub * sigT * sigT + klsum[2 * b]) / 1.0f - 0.5f * dsub;
        const float kl = kl_x + kl_h;
        float err_l = (sums[0][0] + sums[0][1]) * (1.0f - t0), err_q = (sums[1][0] + sums[1][1]) * (1.0f - t0);
        const float l0x_l = 0.5f * sums[0][0] * t0, l0x_q = 0.5f * sums[1][0] * t0, l0h = -(sums[0][2] + sums[1][2]) * t0;
        float loss_t, loss_0, nll;
        if (l2) {
            err_l = err_l / ((float)(3 + P) * nf); err_q = err_q / ((float)(3 + R) * mf);
            loss_t = 0.5f * (err_l + err_q);
            loss_0 = l0x_l / (3.0f * nf) + l0x_q / (3.0f * mf) + l0h;
            nll = loss_t + loss_0 + kl;
        } else {
            loss_t = -T * 0.5f * snrw * (err_l + err_q);
            loss_0 = l0x_l + l0x_q + l0h + tab[TT_NEGLOGC * B + b];
            nll = loss_t + loss_0 + kl - tab[TT_DLOGPX * B + b] - tab[TT_LOGPN * B + b];
        }
        float* o = terms + (size_t)b * TS_COLS;
        o[TS_NLL] = nll; o[TS_ERR_T] = err_l; o[TS_LOSS_0] = loss_0; o[TS_KL] = kl;
        o[TS_ABS_X] = sums[0][3] / (float)max(n, 1); o[TS_ABS_H] = sums[0][4] / (float)max(n, 1);
        o[TS_LOSS_0X] = l0x_l + l0x_q; o[TS_LOSS_0H] = l0h; o[TS_LOSS_T] = loss_t;
        o[TS_ERR_T_Q] = err_q; o[TS_ABS_X_Q] = sums[1][3] / (float)max(m, 1); o[TS_ABS_H_Q] = sums[1][4] / (float)max(m, 1);
    }
}

// means over the batch of every per-sample term column (one workgroup; B is at most a few thousand)
__global__ __launch_bounds__(256) void k_train_means(int B, const float* __restrict__ terms, float* __restrict__ means) {
    __shared__ float red[12];
    for (int c = 0; c < TS_COLS; c += 3) {
        float a = 0.f, b2 = 0.f, c2 = 0.f;
        for (int i = threadIdx.x; i < B; i += 256) {
            const float* o = terms + (size_t)i * TS_COLS + c;
            a += o[0]; b2 += o[1]; c2 += o[2];
        }
        wg_sum3(a, b2, c2, red);
        if (threadIdx.x == 0) { means[c] = a / (float)B; means[c + 1] = b2 / (float)B; means[c + 2] = c2 / (float)B; }
    }
}

void tr_noise(const Layout& lay, const Dims& d, const float* px, const float* poh, const float* qx, const float* qoh, const float* tab,
              const float* eps, float* z_t, float* xh_pocket, float* klsum, hipStream_t s) {
    hipLaunchKernelGGL(k_train_noise, dim3(lay.B), dim3(256), 0, s, lay, d, px, poh, qx, qoh, tab, eps, z_t, xh_pocket, klsum);
}
void tr_loss(const Layout& lay, const Dims& d, int l2, float T, const float* net, const float* eps, const float* z_t, const float* poh,
             const float* tab, const float* klsum, float* terms, float* d_eps, float* means, hipStream_t s) {
    hipLaunchKernelGGL(k_train_loss, dim3(lay.B), dim3(256), 0, s, lay, d, l2, T, net, eps, z_t, poh, tab, klsum, terms, d_eps);
    hipLaunchKernelGGL(k_train_means, dim3(1), dim3(256), 0, s, lay.B, terms, means);
}

void tr_noise_joint(const Layout& lay, const Dims& d, const float* px, const float* poh, const float* qx, const float* qoh, const float* tab,
                    const float* raw_l, const float* raw_q, float* z_l, float* z_q, float* e_l, float* e_q, float* klsum, hipStream_t s) {
    hipLaunchKernelGGL(k_train_noise_joint, dim3(lay.B), dim3(256), 0, s, lay, d, px, poh, qx, qoh, tab, raw_l, raw_q, z_l, z_q, e_l, e_q, klsum);
}
void tr_loss_joint(const Layout& lay, const Dims& d, int l2, float T, const float* net_l, const float* net_q, const float* e_l, const float* e_q,
                   const float* z_l, const float* z_q, const float* poh, const float* qoh, const float* tab, const float* klsum, float* terms,
                   float* d_l, float* d_q, float* means, hipStream_t s) {
    hipLaunchKernelGGL(k_train_loss_joint, dim3(lay.B), dim3(256), 0, s, lay, d, l2, T, net_l, net_q, e_l, e_q, z_l, z_q, poh, qoh, tab, klsum,
                       terms, d_l, d_q);
    hipLaunchKernelGGL(k_train_means, dim3(1), dim3(256), 0, s, lay.B, terms, means);
}
// ------------------------------------------------------------------------------------
// optimizer: AdamW with amsgrad (torch.optim.AdamW semantics, lightning_modules.py:141-143) on the flat buffers,
// with the norm clipping coefficient folded in (clip_grad_norm_: g *= clip when clip < 1).
// ------------------------------------------------------------------------------------
__global__ void k_adamw(size_t n, float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ m,
                        float* __restrict__ v, float* __restrict__ vmax, float lr, float beta1, float beta2, float eps,
                        float weight_decay, float bias1, float bias2_sqrt, float clip, const float* __restrict__ sqnorm,
                        float max_norm, int skip_nonfinite) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (sqnorm) {
        const float sq = sqnorm[0];
        // a step whose forward ran on the half engine and whose gradient is not finite (an activation beyond fp16's range) leaves parameters and
        // moments untouched: the host sees the norm, switches the forward to the bf16 engine and repeats the batch (training.HipTrainer)
        if (skip_nonfinite && !(sq <= 3.0e38f)) return;
        if (max_norm > 0.f) clip = fminf(1.0f, max_norm / (sqrtf(sq) + 1e-6f));  // clip_grad_norm_'s coefficient from the device-side norm
    }
    const float g = grad[i] * clip;
    float p = theta[i];
    p *= 1.0f - lr * weight_decay;
    const float mi = m[i] + (g - m[i]) * (1.0f - beta1);           // lerp, as torch
    const float vi = beta2 * v[i] + (1.0f - beta2) * g * g;
    const float vm = fmaxf(vmax[i], vi);
    m[i] = mi; v[i] = vi; vmax[i] = vm;
    const float denom = sqrtf(vm) / bias2_sqrt + eps;
    theta[i] = p - (lr / bias1) * (mi / denom);
}
// The half engine's range events of a training forward, as one float that may be summed over ranks: TR_EVENT_RESET for a NaN reset (the
// evaluation's guard zeroed the velocities - the fp32 reference would not have seen a NaN there), TR_EVENT_LOW when the tile producers counted
// rows below HALF_LOW_TAU (the counter slot moved since k_low_snap at the forward's start; its low 32 bits suffice: no forward counts 2^32 rows).
#define TR_EVENT_RESET 1.0f
#define TR_EVENT_LOW 4096.0f
__device__ __forceinline__ float range_event(const int* nan_flag, const unsigned long long* counters, const unsigned* snap) {
    return (*nan_flag ? TR_EVENT_RESET : 0.f) + ((unsigned)counters[HALF_LOW_SLOT] != *snap ? TR_EVENT_LOW : 0.f);
}
__global__ void k_low_snap(const unsigned long long* __restrict__ counters, unsigned* __restrict__ snap) { *snap = (unsigned)counters[HALF_LOW_SLOT]; }
__global__ void k_range_event(const int* __restrict__ nan_flag, const unsigned long long* __restrict__ counters, const unsigned* __restrict__ snap,
                              float* __restrict__ out) {
    *out = range_event(nan_flag, counters, snap);
}
// after a forward on the half engine: a range event (this rank's, or - `shared` - the sum over the ranks that the gradient all-reduce carried)
// makes the step's norm non-finite, so that k_adamw skips the update and the host repeats the batch on the bf16 engine; sq[1] keeps the event
// for the host (it reads it with the norm, on the non-finite path only)
__global__ void k_norm_guard(float* __restrict__ sq, const float* __restrict__ shared, const int* __restrict__ nan_flag,
                             const unsigned long long* __restrict__ counters, const unsigned* __restrict__ snap) {
    const float e = shared ? *shared : range_event(nan_flag, counters, snap);
    sq[1] = e;
    if (e > 0.f) sq[0] = __int_as_float(0x7fc00000);
}
void tr_low_snap(const unsigned long long* counters, unsigned* snap, hipStream_t s) { hipLaunchKernelGGL(k_low_snap, dim3(1), dim3(1), 0, s, counters, snap); }
void tr_range_event(const int* nan_flag, const unsigned long long* counters, const unsigned* snap, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_range_event, dim3(1), dim3(1), 0, s, nan_flag, counters, snap, out);
}
void tr_norm_guard(float* sq, const float* shared, const int* nan_flag, const unsigned long long* counters, const unsigned* snap, hipStream_t s) {
    hipLaunchKernelGGL(k_norm_guard, dim3(1), dim3(1), 0, s, sq, shared, nan_flag, counters, snap);
}
__global__ __launch_bounds__(256) void k_sqsum(size_t n, const float* __restrict__ x, float* __restrict__ out) {
    // one atomic per workgroup: thousands of waves adding into the same address serialise (44 us for 3M elements before)
    __shared__ float red[4];
    float v = 0.f;
    const size_t n4 = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? n / 4 : 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 q = reinterpret_cast<const float4*>(x)[i];
        v += q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    }
    for (size_t i = 4 * n4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) v += x[i] * x[i];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, (red[0] + red[1]) + (red[2] + red[3]));
}
#define EW_GRID(n) dim3((unsigned)(((size_t)(n) + 255) / 256)), dim3(256)
void tr_adamw(size_t n, float* theta, const float* grad, float* m, float* v, float* vmax, float lr, float b1, float b2,
              float eps, float wd, float bias1, float bias2_sqrt, float clip, hipStream_t s, const float* sqnorm,
              float max_norm, int skip_nonfinite) {
    if (n) hipLaunchKernelGGL(k_adamw, EW_GRID(n), 0, s, n, theta, grad, m, v, vmax, lr, b1, b2, eps, wd, bias1, bias2_sqrt, clip, sqnorm, max_norm, skip_nonfinite);
}
void tr_sqsum(size_t n, const float* x, float* out, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_sqsum, dim3((unsigned)(n / 8192 + 1 > 512 ? 512 : n / 8192 + 1)), dim3(256), 0, s, n, x, out);
}
