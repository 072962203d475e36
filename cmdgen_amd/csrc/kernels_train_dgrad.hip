// kernels_train_dgrad.hip - the data-gradient and edge-list kernels of the training step's backward pass: data gradients on the split-bf16
// engine (k_dgrad_split; k_dgrad_tail with the whole tail pass of an edge list inside), the stand-alone tail pass (k_edge_tail_bwd), the
// gate / head adjoints and their parameter reductions; each with its launcher.  The per-edge coordinate adjoint and the slice reduction
// they are composed of: cmdgen_train_parts.h.  (The small element-wise adjoints: kernels_train_adjoint.hip.)
// the data-gradient kernels keep the plane GEMM's loads in a burst per k-block: pinned one by one under the MFMAs (the sampler's edge
// kernels: -6 % per launch) k_dgrad_split<32,3> takes 1.23 instead of 0.95 ms per three steps (profiles/r03_n_wgrad.txt).  This unit alone
// instantiates dgrad_tile_gemm, so the switch is set here and nowhere else.
#define CMDGEN_PLANE_PIN 0
#include "cmdgen_train_parts.h"

// ------------------------------------------------------------------------------------
// Data gradients on the split-bf16 matrix engine (cmdgen_split.h: fp32-accurate, six bf16 MFMAs per fp32 product):
//   Y[M][256] (+)= ( A0[M][256] W0 + A1[M][256] W1 ) / div  (* SiLU'(pre[M][256]))
// where W0 / W1 are 256 x 256 sub-blocks W[:, col0 : col0 + 256] of nn.Linear weights (dX = dY W), streamed as split
// fragment packs of their TRANSPOSES (k_repack_split_t, re-made every step from the parameters the optimizer has just
// updated).  All [.,256] x [256,256] products of the backward pass have this shape: the second layer of the edge /
// coordinate MLP over the edges, and the seven node-level products of a block - the two halves of edge_mlp.0 and
// coord_mlp.0 (A0 = dP, A1 = dQ: one launch instead of two), node_mlp.2, and the two halves of node_mlp.0.
// One workgroup per MT rows: the A tile is staged once in LDS as fp32, every wave splits the fragments it reads in
// registers in the shadow of the MFMAs (tile_gemm_rsplit), the weight fragments stream from L2.
// ------------------------------------------------------------------------------------
// the GEMM part: acc = A0[row0 .. row0+MT) W0 (+ A1 W1).  The A operand lies in LDS as three bf16 planes [MT][136] of one
// half of the k range at a time (tile_gemm_planes): the thread that loads an element splits it once; the next half's rows
// are requested before this half's MFMAs start.  Ends with a barrier (the planes may be overwritten).
template <int MT, int NPC>
__device__ __forceinline__ void dgrad_tile_gemm(unsigned short* planes, int M, int row0, const float* __restrict__ A0,
                                                const void* __restrict__ W0, const float* __restrict__ A1,
                                                const void* __restrict__ W1, sf32x16 (&acc)[MT / 32][2]) {
    constexpr int HH = 256, PLDA = SPLIT_PLANE_LDA(HH / 2), PE = MT * PLDA, NP = MT / 8;
    const int tid = threadIdx.x, wave = tid >> 6;
    const int c4 = tid & 31, rsub = tid >> 5;            // 32 lanes x 16 bytes = one half row, 8 rows per pass
    SCarry carry;
    const int nstage = A1 ? 4 : 2;                        // (source, half)
    auto frag_of = [&](int st) { return sfrag_ptr((st >> 1) ? W1 : W0, HH / 16, (st & 1) * (HH / 32), wave); };
    split_prefetch<NPC>(frag_of(0), carry);
    float4 v[NP];
    auto fetch = [&](int st) {
        const float* A = (st >> 1) ? A1 : A0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int r = row0 + p * 8 + rsub;
            v[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < M) v[p] = *reinterpret_cast<const float4*>(A + (size_t)r * HH + (st & 1) * (HH / 2) + 4 * c4);
        }
    };
    fetch(0);
#pragma unroll
    for (int m = 0; m < MT / 32; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
#pragma unroll 1
    for (int st = 0; st < nstage; ++st) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if constexpr (NPC == 3) split_store4(planes, PE, (p * 8 + rsub) * PLDA + 4 * c4, v[p]);
            else *reinterpret_cast<uint2*>(planes + (p * 8 + rsub) * PLDA + 4 * c4) = make_uint2(cvt_pk_bf16(v[p].x, v[p].y), cvt_pk_bf16(v[p].z, v[p].w));
        }
        __syncthreads();
        if (st + 1 < nstage) fetch(st + 1);
        tile_gemm_planes<MT, HH / 32, NPC>(planes, PE, PLDA, frag_of(st), frag_of(st + 1 < nstage ? st + 1 : st), acc, carry);
        __syncthreads();
    }
}

template <int MT, int NPC>
__global__ __launch_bounds__(256, 2) void k_dgrad_split(int M, const float* __restrict__ A0, const void* __restrict__ W0,
                                                        const float* __restrict__ A1, const void* __restrict__ W1,
                                                        float* Y, int accumulate, float div,
                                                        const float* __restrict__ pre, const void* __restrict__ W0b,
                                                        float* __restrict__ Yb, int accumulate_b, float div_b, const float* Yin,
                                                        const float* __restrict__ rowdiv_b) {
    // gridDim.y = 2: a second product of the same A0 (W0b -> Yb; the two halves of node_mlp.0 share dpre3) in the same launch
    // Yin: the running value an accumulating product adds to (Y itself, or another buffer: Y = Yin + product, out of place)
    // rowdiv_b: per-row divisor of the second product instead of div_b (aggregation 'mean': the receiver's edge count)
    const float* rowdiv = nullptr;
    if (blockIdx.y) { W0 = W0b; Y = Yb; Yin = Yb; accumulate = accumulate_b; div = div_b; rowdiv = rowdiv_b; }
    constexpr int HH = 256, PLDA = SPLIT_PLANE_LDA(HH / 2), PE = MT * PLDA;
    constexpr int LDO = HH + 4, SMEM = 3 * PE * 2 > 32 * LDO * 4 ? 3 * PE * 2 : 32 * LDO * 4;   // planes / 32-row fp32 output image
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row0 = blockIdx.x * MT;
    sf32x16 acc[MT / 32][2];
    dgrad_tile_gemm<MT, NPC>(reinterpret_cast<unsigned short*>(smem), M, row0, A0, W0, A1, W1, acc);
    // Epilogue through LDS, 32 rows at a time (the fp32 image of 32 rows, 33 KB, aliases the planes): whole 1 KB rows leave
    // as 16-byte pieces, and SiLU'(pre) / the running value of Y are read the same way.  Accumulator element r of tile
    // (m, n) is row m*32 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column wave*64 + n*32 + (lane & 31).
    float* obuf = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int m = 0; m < MT / 32; ++m) {
        if (m) __syncthreads();
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                obuf[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * LDO + wave * 64 + n * 32 + (lane & 31)] = acc[m][n][r];
        __syncthreads();
        const int q4 = tid & 63, rs = tid >> 6;          // a wave writes one row per pass
        float4 pv[8], yv[8];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int row = row0 + m * 32 + p * 4 + rs;
            if (row < M) {
                if (pre) pv[p] = reinterpret_cast<const float4*>(pre + (size_t)row * HH)[q4];
                if (accumulate) yv[p] = reinterpret_cast<const float4*>(Yin + (size_t)row * HH)[q4];
            }
        }
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int rl = p * 4 + rs, row = row0 + m * 32 + rl;
            if (row < M) {
                float4 x = *reinterpret_cast<const float4*>(obuf + rl * LDO + 4 * q4);
                if (rowdiv) { const float dvr = rowdiv[row]; x.x = x.x / dvr; x.y = x.y / dvr; x.z = x.z / dvr; x.w = x.w / dvr; }
                else if (div != 1.0f) { x.x = x.x / div; x.y = x.y / div; x.z = x.z / div; x.w = x.w / div; }
                if (pre) { x.x *= dsilu(pv[p].x); x.y *= dsilu(pv[p].y); x.z *= dsilu(pv[p].z); x.w *= dsilu(pv[p].w); }
                if (accumulate) { x.x += yv[p].x; x.y += yv[p].y; x.z += yv[p].z; x.w += yv[p].w; }
                reinterpret_cast<float4*>(Y + (size_t)row * HH)[q4] = x;
            }
        }
    }
}
void cmdgen_dgrad_split(int M, const float* A0, const void* W0, const float* A1, const void* W1, float* Y, bool accumulate, float div,
                        const float* pre, hipStream_t s, const TrainTune& tune, int pieces, const void* W0b, float* Yb,
                        bool accumulate_b, float div_b, int force_mt, const float* Yin, const float* rowdiv_b) {
    if (M <= 0) return;
    if (!Yin) Yin = Y;
    const int mt = plan_dgrad(M, tune, force_mt);
    typedef void (*Kernel)(int, const float*, const void*, const float*, const void*, float*, int, float, const float*, const void*, float*, int, float,
                           const float*, const float*);
    static const Kernel tab[2][2] = {{k_dgrad_split<32, 1>, k_dgrad_split<32, 3>}, {k_dgrad_split<64, 1>, k_dgrad_split<64, 3>}};     // [64 rows][three pieces]
    hipLaunchKernelGGL(tab[mt == 64][pieces == 3], dim3((M + mt - 1) / mt, W0b ? 2 : 1), dim3(256), 0, s, M, A0, W0, A1, W1, Y, accumulate ? 1 : 0, div, pre,
                       W0b, Yb, accumulate_b ? 1 : 0, div_b, Yin, rowdiv_b);
}

// ------------------------------------------------------------------------------------
// The same adjoint in ONE pass over pre2, together with the two reductions that used to follow it (k_colsum4 over m2
// with weights dz, k_sum over dz): m2 = SiLU(pre2) is recomputed with the forward's own silu_f instead of being read
// (the forward no longer stores it), d att_mlp.weight[c] += sum_e dz_e m2[e][c] and d att_mlp.bias += sum_e dz_e are
// accumulated per workgroup (32 consecutive edges, 8 per wave, a lane owns four consecutive columns) and written to a
// scratch row; k_partial_reduce adds the rows up.  H <= 256, H % 4 == 0.
// ------------------------------------------------------------------------------------
#define GATE_EPW 8
__global__ __launch_bounds__(256) void k_gate_bwd(int E, int H, const int* __restrict__ row, const float* __restrict__ pre2,
                                                  const float* __restrict__ wa, const float* __restrict__ z, int attention,
                                                  const float* __restrict__ dagg, float* __restrict__ dpre2,
                                                  float* __restrict__ scratch /* [workgroups][H + 4] */,
                                                  float4* __restrict__ zero, size_t zero_n4) {
    __shared__ float red[4][260];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // side duty: clear the buffer the NEXT kernel of the pass accumulates into (dP | dQ) - one memset launch less per list
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < zero_n4; i += (size_t)gridDim.x * 256) zero[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool on = 4 * lane < H;
    const int e0 = blockIdx.x * (4 * GATE_EPW) + wave * GATE_EPW, e1 = min(E, e0 + GATE_EPW);
    float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f), cs = w4;
    if (on && attention) w4 = reinterpret_cast<const float4*>(wa)[lane];
    float sdz = 0.f;
    float4 pv[GATE_EPW], gv[GATE_EPW];
    float zv[GATE_EPW];
#pragma unroll
    for (int k = 0; k < GATE_EPW; ++k) {            // all rows of the wave requested before the first is used
        const int e = e0 + k;
        pv[k] = gv[k] = make_float4(0.f, 0.f, 0.f, 0.f); zv[k] = 0.f;
        if (e < e1) {
            if (on) {
                pv[k] = reinterpret_cast<const float4*>(pre2 + (size_t)e * H)[lane];
                gv[k] = reinterpret_cast<const float4*>(dagg + (size_t)row[e] * H)[lane];
            }
            if (attention) zv[k] = z[e];
        }
    }
#pragma unroll
    for (int k = 0; k < GATE_EPW; ++k) {
        const int e = e0 + k;
        if (e < e1) {                                // wave-uniform
            const float4 p = pv[k], g = gv[k];
            float att = 1.0f, dz = 0.f;
            if (attention) {
                const float4 m = make_float4(silu_f(p.x), silu_f(p.y), silu_f(p.z), silu_f(p.w));
                att = 1.0f / (1.0f + expf(-zv[k]));
                dz = wave_sum(g.x * m.x + g.y * m.y + g.z * m.z + g.w * m.w) * att * (1.0f - att);
                cs.x += dz * m.x; cs.y += dz * m.y; cs.z += dz * m.z; cs.w += dz * m.w;
                sdz += dz;
            }
            if (on) {
                float4 o;
                o.x = (g.x * att + dz * w4.x) * dsilu(p.x); o.y = (g.y * att + dz * w4.y) * dsilu(p.y);
                o.z = (g.z * att + dz * w4.z) * dsilu(p.z); o.w = (g.w * att + dz * w4.w) * dsilu(p.w);
                reinterpret_cast<float4*>(dpre2 + (size_t)e * H)[lane] = o;
            }
        }
    }
    if (!attention) return;
    *reinterpret_cast<float4*>(&red[wave][4 * lane]) = cs;
    if (lane == 0) red[wave][256] = sdz;
    __syncthreads();
    float* out = scratch + (size_t)blockIdx.x * (H + 4);
    for (int c = threadIdx.x; c < H; c += 256) out[c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    if (threadIdx.x == 0) out[H] = (red[0][256] + red[1][256]) + (red[2][256] + red[3][256]);
}

// dpre7[e][c] = dphi_e w5[c] SiLU'(pre7[e][c]) and, in the same pass, the partial sums of d coord_mlp.4.weight[c] =
// sum_e dphi_e SiLU(pre7[e][c]) (c2 is recomputed, not read); same workgroup shape and scratch layout as k_gate_bwd.
__global__ __launch_bounds__(256) void k_head_bwd(int E, int H, const float* __restrict__ dphi, const float* __restrict__ w5,
                                                  const float* __restrict__ pre7, float* __restrict__ dpre7,
                                                  float* __restrict__ scratch /* [workgroups][H + 4] */,
                                                  float4* __restrict__ zero, size_t zero_n4, CoordOutArgs co) {
    __shared__ float red[4][260];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < zero_n4; i += (size_t)gridDim.x * 256) zero[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool on = 4 * lane < H;
    const int e0 = blockIdx.x * (4 * GATE_EPW) + wave * GATE_EPW, e1 = min(E, e0 + GATE_EPW);
    // co.row: dphi is not read but formed here, by lane k for the wave's k-th edge (coord_out_edge), and dcd written
    float my_dphi = 0.f;
    if (co.row && lane < GATE_EPW && e0 + lane < e1) my_dphi = coord_out_edge(co, e0 + lane);
    float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f), cs = w4;
    if (on) w4 = reinterpret_cast<const float4*>(w5)[lane];
    float4 pv[GATE_EPW]; float sv[GATE_EPW];
#pragma unroll
    for (int k = 0; k < GATE_EPW; ++k) {
        const int e = e0 + k;
        pv[k] = make_float4(0.f, 0.f, 0.f, 0.f); sv[k] = 0.f;
        if (e < e1 && on) pv[k] = reinterpret_cast<const float4*>(pre7 + (size_t)e * H)[lane];
        if (!co.row && e < e1) sv[k] = dphi[e];
    }
    if (co.row) {
#pragma unroll
        for (int k = 0; k < GATE_EPW; ++k) sv[k] = __shfl(my_dphi, k);
    }
#pragma unroll
    for (int k = 0; k < GATE_EPW; ++k) {
        const int e = e0 + k;
        if (e < e1 && on) {
            const float4 p = pv[k]; const float se = sv[k];
            cs.x += se * silu_f(p.x); cs.y += se * silu_f(p.y); cs.z += se * silu_f(p.z); cs.w += se * silu_f(p.w);
            reinterpret_cast<float4*>(dpre7 + (size_t)e * H)[lane] =
                make_float4(se * w4.x * dsilu(p.x), se * w4.y * dsilu(p.y), se * w4.z * dsilu(p.z), se * w4.w * dsilu(p.w));
        }
    }
    *reinterpret_cast<float4*>(&red[wave][4 * lane]) = cs;
    __syncthreads();
    float* out = scratch + (size_t)blockIdx.x * (H + 4);
    for (int c = threadIdx.x; c < H; c += 256) out[c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// out_w[c] += sum over workgroups of scratch[wg][c] (c < H), out_b[0] += sum of scratch[wg][H] (when out_b).  grid
// ((H + 1 + 63) / 64, slices): every workgroup sums one slice of the rows for 64 columns and adds its result with one atomic.
__global__ __launch_bounds__(256) void k_partial_reduce(int nwg, int H, const float* __restrict__ scratch, float* __restrict__ out_w,
                                                        float* __restrict__ out_b) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    reduce_slice(nwg, gridDim.y, blockIdx.y, scratch, H + 4, c, c < H + (out_b ? 1 : 0), [&](float t) { atomicAdd(c < H ? out_w + c : out_b, t); });
}

// ------------------------------------------------------------------------------------
// k_edge_tail_bwd: everything the backward pass does with g = dL/d pre1 [E][H] of an edge list (pre1 = P[row] + Q[col]
// + w_r r + w_d d0, the first layer of the edge / coordinate MLP), in ONE pass over g instead of seven launches:
//   dP[row] += g (adjoint of the gather of P; rows are sorted, so a wave sums a receiver's run in registers and adds
//   once per run), dQ[col] += g (atomics), dW[:, 2H] += sum_e r_e g_e and dW[:, 2H+1] += sum_e d0_e g_e (the radial /
//   d0 columns of the Linear, strided by ldw), dr_e = g_e . w_r, and the geometry adjoint of k_geom_bwd for that dr_e
//   (plus dcd_e for the coordinate list) into dX.  A wave takes TAIL_EPW consecutive edges (a workgroup 4 x that).
//   INP (input gradients, cmdgen_train_backward_inputs only): also dd0[e] += g_e . w_d, the adjoint of the edge's d0 feature (its geometry
//   adjoint into the input positions runs once after the last block: k_d0_adjoint); the caller passes n_moving = N there.
// ------------------------------------------------------------------------------------
#define TAIL_EPW 8              // edges per wave: short serial runs, thousands of waves in flight
template <bool INP = false>
__global__ __launch_bounds__(256) void k_edge_tail_bwd(int E, int H, const int* __restrict__ row, const int* __restrict__ col,
                                                       const float* __restrict__ g, const float* __restrict__ d0,
                                                       const float* __restrict__ Wcol /* W + 2H, stride ldw */, int ldw,
                                                       const float4* __restrict__ X, float norm_constant,
                                                       const float4* __restrict__ dcd, int n_moving,
                                                       float* __restrict__ dP, float* __restrict__ dQ,
                                                       float* __restrict__ scratch /* [workgroups][2][H] */, float* __restrict__ dX,
                                                       const float* __restrict__ Wd /* d0 column, stride ldw */, float* __restrict__ dd0) {
    __shared__ float red[2][4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // a lane owns columns lane, lane + 64, lane + 128, lane + 192: every load / atomic of the wave is one contiguous
    // 256-byte piece of a row (the shape float atomics run at full rate in, MI355X_MICROARCH.md "Global float atomics")
    const int NC = (H + 63) / 64;
    const int e0 = blockIdx.x * (4 * TAIL_EPW) + wave * TAIL_EPW, e1 = min(E, e0 + TAIL_EPW);
    const int ne = max(e1 - e0, 0);
    float wr[4], wd[4], accR[4], accD[4], run[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = lane + 64 * q;
        wr[q] = (q < NC && c < H) ? Wcol[(size_t)c * ldw] : 0.f;
        wd[q] = (INP && q < NC && c < H) ? Wd[(size_t)c * ldw] : 0.f;
        accR[q] = accD[q] = run[q] = 0.f;
    }
    // lane l < ne owns edge e0 + l for the per-edge scalars: indices, geometry, and later the geometry adjoint
    int my_i = -1, my_j = -1; float my_r = 0.f, my_d0 = 0.f, dxl = 0.f, dyl = 0.f, dzl = 0.f;
    if (lane < ne) {
        my_i = row[e0 + lane]; my_j = col[e0 + lane]; my_d0 = d0[e0 + lane];
        const float4 a = X[my_i], b = X[my_j];
        dxl = a.x - b.x; dyl = a.y - b.y; dzl = a.z - b.z;
        my_r = dxl * dxl + dyl * dyl + dzl * dzl;
    }
    float my_gr = 0.f, my_gd = 0.f;
    int cur = __shfl(my_i, 0);
#pragma unroll
    for (int k = 0; k < TAIL_EPW; ++k) {
        if (k < ne) {                                        // wave-uniform
            const int e = e0 + k;
            const int i = __shfl(my_i, k), j = __shfl(my_j, k);
            const float r = __shfl(my_r, k), dd = __shfl(my_d0, k);
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int c = lane + 64 * q; v[q] = (c < H) ? g[(size_t)e * H + c] : 0.f; }
            if (i != cur) {                                  // the receiver's run ended: one add per run
#pragma unroll
                for (int q = 0; q < 4; ++q) { const int c = lane + 64 * q; if (c < H) atomicAdd(dP + (size_t)cur * H + c, run[q]); run[q] = 0.f; }
                cur = i;
            }
            float dot = 0.f, dotd = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = lane + 64 * q;
                accR[q] += r * v[q]; accD[q] += dd * v[q]; run[q] += v[q]; dot += v[q] * wr[q];
                if (INP) dotd += v[q] * wd[q];
                if (c < H) atomicAdd(dQ + (size_t)j * H + c, v[q]);
            }
            const float gr = wave_sum(dot);                  // dL/d radial of this edge
            if (lane == k) my_gr = gr;
            if (INP) { const float gd = wave_sum(dotd); if (lane == k) my_gd = gd; }      // dL/d d0 of this edge
        }
    }
    if (INP && lane < ne) dd0[e0 + lane] += my_gd;        // one lane per edge: every block's list launch adds in stream order
    if (ne > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int c = lane + 64 * q; if (c < H) atomicAdd(dP + (size_t)cur * H + c, run[q]); }
    }
    if (lane < ne && my_i != my_j) {                         // geometry adjoint, one lane per edge (as k_geom_bwd)
        const float sq = sqrtf(my_r + 1e-8f), den = sq + norm_constant;
        float gx = 0.f, gy = 0.f, gz = 0.f, gr = my_gr;
        if (dcd) {
            const float4 d = dcd[e0 + lane];
            gx = d.x / den; gy = d.y / den; gz = d.z / den;
            const float dden = -(d.x * dxl + d.y * dyl + d.z * dzl) / (den * den);
            gr += dden * 0.5f / sq;
        }
        gx += 2.0f * dxl * gr; gy += 2.0f * dyl * gr; gz += 2.0f * dzl * gr;
        if (my_i < n_moving) { float* p = dX + (size_t)my_i * 4; atomicAdd(p, gx); atomicAdd(p + 1, gy); atomicAdd(p + 2, gz); }
        if (my_j < n_moving) { float* p = dX + (size_t)my_j * 4; atomicAdd(p, -gx); atomicAdd(p + 1, -gy); atomicAdd(p + 2, -gz); }
    }
    // column sums: per-workgroup partials go to a scratch row (plain stores); k_tail_colsum_reduce adds them up.  (Hundreds
    // of workgroups adding into the same 2H addresses with float atomics serialise at the memory side.)
#pragma unroll
    for (int q = 0; q < 4; ++q) { red[0][wave][lane + 64 * q] = accR[q]; red[1][wave][lane + 64 * q] = accD[q]; }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 2 * H; idx += 256) {
        const int which = idx / H, c = idx - which * H;
        scratch[((size_t)blockIdx.x * 2 + which) * H + c] = (red[which][0][c] + red[which][1][c]) + (red[which][2][c] + red[which][3][c]);
    }
}
// ------------------------------------------------------------------------------------
// k_dgrad_tail: the data gradient through the second layer of an edge / coordinate MLP AND everything k_edge_tail_bwd does
// with its result, in one kernel: g = (dY W2) * SiLU'(pre1) of a 32-edge tile never leaves the chip (one [E,256] tensor
// less written and read per list and block).  GEMM as k_dgrad_split<32>; the accumulators go to LDS, every wave applies
// SiLU'(pre1) to the eight rows it owns (whole-row reads of pre1) and then runs the tail on the same rows: receiver runs
// into dP, dQ atomics, the radial / d0 column partial sums, dL/d radial and the geometry adjoint - lanes own columns
// lane + 64 q exactly as in k_edge_tail_bwd (contiguous 256-byte atomics).  Scratch layout and reduce kernel are shared.
// The tail is typed out a second time here, statement for statement k_edge_tail_bwd's with the row read from the LDS image and H = 256:
// composed from shared parts this kernel came out 5 to 14 instructions longer whichever way the parts were cut, so both
// keep their bodies.  A change to the tail's arithmetic is made in both; the option dgrad_tail = 0 runs the other copy at this width, and
// tests/test_hip_train.py::test_unfused_edge_tail_agrees_with_the_fused_one_at_width_256 holds the two against each other.
// ------------------------------------------------------------------------------------
#ifndef CMDGEN_TAIL_STAMPS
#define CMDGEN_TAIL_STAMPS 0
#endif
struct TailArgs {
    const int* row; const int* col; const float* d0; const float* Wcol; int ldw;
    const float4* X; float norm_constant; const float4* dcd; int n_moving;
    float* dP; float* dQ; float* scratch; float* dX;
    unsigned long long* dbg;      // diagnostic build (-DCMDGEN_TAIL_STAMPS=1): per-phase cycle sums [wave][8], [32 + wave] lifetimes, [40] workgroups; else unused
    const float* Wd; float* dd0;  // INP only: the d0 column (stride ldw) and the per-edge d0 adjoint it adds into (as k_edge_tail_bwd<true>)
};
template <int NPC, bool INP = false>
__global__ __launch_bounds__(256, 3) void k_dgrad_tail(int M, const float* __restrict__ A0, const void* __restrict__ W0,
                                                       const float* __restrict__ pre, TailArgs ta) {
    constexpr int MT = 32, HH = 256, PLDA = SPLIT_PLANE_LDA(HH / 2), PE = MT * PLDA;
    constexpr int LDO = HH + 4, SMEM = 3 * PE * 2 > 32 * LDO * 4 ? 3 * PE * 2 : 32 * LDO * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row0 = blockIdx.x * MT;
#if CMDGEN_TAIL_STAMPS == 1
    unsigned long long st_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_t = __builtin_amdgcn_s_memtime();
    const unsigned long long st_begin = st_t;
#define TSTAMP(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); st_[i] += n_ - st_t; st_t = n_; } while (0)
#else
#define TSTAMP(i) do {} while (0)
#endif
    // the tail's per-edge scalars: requested before the GEMM, used after it
    const int e0 = row0 + wave * 8, ne = max(0, min(8, M - e0));
    // (the positions - a second, dependent round trip - are requested after the GEMM, together with the pre1 rows: in front of the GEMM
    // their difference stood in every tile's critical path; profiles/r05_ah_tail_stamps.txt)
    int my_i = -1, my_j = -1; float my_r = 0.f, my_d0 = 0.f, dxl = 0.f, dyl = 0.f, dzl = 0.f;
    if (lane < ne) { my_i = ta.row[e0 + lane]; my_j = ta.col[e0 + lane]; my_d0 = ta.d0[e0 + lane]; }
    float wr[4], wd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) wr[q] = ta.Wcol[(size_t)(lane + 64 * q) * ta.ldw];
    if (INP) {
#pragma unroll
        for (int q = 0; q < 4; ++q) wd[q] = ta.Wd[(size_t)(lane + 64 * q) * ta.ldw];
    }
    sf32x16 acc[1][2];
    TSTAMP(0);
    dgrad_tile_gemm<MT, NPC>(reinterpret_cast<unsigned short*>(smem), M, row0, A0, W0, nullptr, nullptr, acc);
    TSTAMP(1);
    float* obuf = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            obuf[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * LDO + wave * 64 + n * 32 + (lane & 31)] = acc[0][n][r];
    __syncthreads();
    TSTAMP(2);
    // SiLU'(pre1) on this wave's rows 8 wave .. 8 wave + 7 (the same rows its tail walks: no barrier in between)
    {
        float4 xa = make_float4(0.f, 0.f, 0.f, 0.f), xb = xa;
        if (lane < ne) { xa = ta.X[my_i]; xb = ta.X[my_j]; }
        float4 pv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) if (k < ne) pv[k] = reinterpret_cast<const float4*>(pre + (size_t)(e0 + k) * HH)[lane];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < ne) {
                float4* cell = reinterpret_cast<float4*>(obuf + (wave * 8 + k) * LDO + 4 * lane);
                float4 x = *cell;
                x.x *= dsilu(pv[k].x); x.y *= dsilu(pv[k].y); x.z *= dsilu(pv[k].z); x.w *= dsilu(pv[k].w);
                *cell = x;
            }
        dxl = xa.x - xb.x; dyl = xa.y - xb.y; dzl = xa.z - xb.z;
        my_r = dxl * dxl + dyl * dyl + dzl * dzl;
    }
    TSTAMP(3);
    float accR[4] = {0.f, 0.f, 0.f, 0.f}, accD[4] = {0.f, 0.f, 0.f, 0.f}, run[4] = {0.f, 0.f, 0.f, 0.f};
    float my_gr = 0.f, my_gd = 0.f;
    int cur = __shfl(my_i, 0);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < ne) {                                        // wave-uniform
            const int i = __shfl(my_i, k), j = __shfl(my_j, k);
            const float r = __shfl(my_r, k), dd = __shfl(my_d0, k);
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = obuf[(wave * 8 + k) * LDO + lane + 64 * q];
            if (i != cur) {                                  // the receiver's run ended: one add per run
#pragma unroll
                for (int q = 0; q < 4; ++q) { atomicAdd(ta.dP + (size_t)cur * HH + lane + 64 * q, run[q]); run[q] = 0.f; }
                cur = i;
            }
            float dot = 0.f, dotd = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                accR[q] += r * v[q]; accD[q] += dd * v[q]; run[q] += v[q]; dot += v[q] * wr[q];
                if (INP) dotd += v[q] * wd[q];
                atomicAdd(ta.dQ + (size_t)j * HH + lane + 64 * q, v[q]);
            }
            const float gr = wave_sum(dot);                  // dL/d radial of this edge
            if (lane == k) my_gr = gr;
            if (INP) { const float gd = wave_sum(dotd); if (lane == k) my_gd = gd; }      // dL/d d0 of this edge
        }
    }
    if (INP && lane < ne) ta.dd0[e0 + lane] += my_gd;
    TSTAMP(4);
    if (ne > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) atomicAdd(ta.dP + (size_t)cur * HH + lane + 64 * q, run[q]);
    }
    if (lane < ne && my_i != my_j) {                         // geometry adjoint, one lane per edge (as k_geom_bwd)
        const float sq = sqrtf(my_r + 1e-8f), den = sq + ta.norm_constant;
        float gx = 0.f, gy = 0.f, gz = 0.f, gr = my_gr;
        if (ta.dcd) {
            const float4 d = ta.dcd[e0 + lane];
            gx = d.x / den; gy = d.y / den; gz = d.z / den;
            const float dden = -(d.x * dxl + d.y * dyl + d.z * dzl) / (den * den);
            gr += dden * 0.5f / sq;
        }
        gx += 2.0f * dxl * gr; gy += 2.0f * dyl * gr; gz += 2.0f * dzl * gr;
        if (my_i < ta.n_moving) { float* p = ta.dX + (size_t)my_i * 4; atomicAdd(p, gx); atomicAdd(p + 1, gy); atomicAdd(p + 2, gz); }
        if (my_j < ta.n_moving) { float* p = ta.dX + (size_t)my_j * 4; atomicAdd(p, -gx); atomicAdd(p + 1, -gy); atomicAdd(p + 2, -gz); }
    }
    TSTAMP(5);
    // column sums: per-workgroup partials to the scratch row (k_tail_colsum_reduce adds them up)
    __syncthreads();                                         // every wave is done with the output image
    float* red = obuf;                                       // [2][4][256]
#pragma unroll
    for (int q = 0; q < 4; ++q) { red[(0 * 4 + wave) * 256 + lane + 64 * q] = accR[q]; red[(1 * 4 + wave) * 256 + lane + 64 * q] = accD[q]; }
    __syncthreads();
    for (int idx = tid; idx < 2 * HH; idx += 256) {
        const int which = idx / HH, c = idx - which * HH;
        ta.scratch[((size_t)blockIdx.x * 2 + which) * HH + c] =
            (red[(which * 4 + 0) * 256 + c] + red[(which * 4 + 1) * 256 + c]) + (red[(which * 4 + 2) * 256 + c] + red[(which * 4 + 3) * 256 + c]);
    }
    TSTAMP(6);
#if CMDGEN_TAIL_STAMPS == 1
    if (ta.dbg && lane == 0 && (blockIdx.x & 3) == 0) {
        for (int i = 0; i < 7; ++i) atomicAdd(&ta.dbg[wave * 8 + i], st_[i]);
        atomicAdd(&ta.dbg[32 + wave], __builtin_amdgcn_s_memtime() - st_begin);
        if (wave == 0) atomicAdd(&ta.dbg[40], 1ull);
    }
#endif
#undef TSTAMP
}
// dWcol[which + c * ldw] += sum over workgroups of scratch[wg][which][c].  grid (H / 64, 2, slices): every workgroup sums
// one slice of the partial rows for 64 columns (4 rows in flight per column) and adds its result with one atomic.
__global__ __launch_bounds__(256) void k_tail_colsum_reduce(int nwg, int H, const float* __restrict__ scratch,
                                                            float* __restrict__ dWcol, int ldw) {
    const int which = blockIdx.y, c = blockIdx.x * 64 + (threadIdx.x & 63);
    reduce_slice(nwg, gridDim.z, blockIdx.z, scratch, 2 * (size_t)H, (size_t)which * H + c, c < H, [&](float t) { atomicAdd(dWcol + which + (size_t)c * ldw, t); });
}

// ------------------------------------------------------------------------------------
// launch helpers (C++ linkage, used by cmdgen_train.hip)
// ------------------------------------------------------------------------------------
// The two reductions of an edge list in one launch: blockIdx.y = 0 is k_partial_reduce's job (gate / head partial sums,
// scratch rows of H + 4 floats), blockIdx.y = 1, 2 are k_tail_colsum_reduce's (radial / d0 column partials, rows of 2 H).
__global__ __launch_bounds__(256) void k_reduce_pair(int nwg_a, int H, const float* __restrict__ scratch_a, float* __restrict__ out_w,
                                                     float* __restrict__ out_b, int nwg_t, const float* __restrict__ scratch_t,
                                                     float* __restrict__ dWcol, int ldw) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const bool job_a = blockIdx.y == 0;
    if (job_a && !out_w) return;                 // (a model without attention has no gate parameters)
    const int which = (int)blockIdx.y - 1;
    reduce_slice(job_a ? nwg_a : nwg_t, gridDim.z, blockIdx.z, job_a ? scratch_a : scratch_t, job_a ? (size_t)(H + 4) : 2 * (size_t)H,
                 job_a ? (size_t)c : (size_t)which * H + c, c < (job_a ? H + (out_b ? 1 : 0) : H), [&](float t) {
        if (job_a) atomicAdd(c < H ? out_w + c : out_b, t);
        else atomicAdd(dWcol + which + (size_t)c * ldw, t);
    });
}
void tr_reduce_pair(int E, int H, const float* scratch_a, float* out_w, float* out_b, const float* scratch_t, float* dWcol, int ldw, hipStream_t s) {
    if (E <= 0) return;
    const int nwg = (E + 31) / 32;               // both producers take 32 edges per workgroup
    hipLaunchKernelGGL(k_reduce_pair, dim3((H + 1 + 63) / 64, 3, min(32, (nwg + 15) / 16)), dim3(256), 0, s, nwg, H, scratch_a, out_w, out_b,
                       nwg, scratch_t, dWcol, ldw);
}
size_t tr_partial_scratch_floats(size_t E, size_t H) { return ((E + 4 * GATE_EPW - 1) / (4 * GATE_EPW)) * (H + 4); }
// the attention gate's adjoint with its two parameter gradients (d_wa [H], d_ba [1]; ignored without attention)
void tr_gate_bwd(int E, int H, const int* row, const float* pre2, const float* wa, const float* z, int attention, const float* dagg,
                 float* dpre2, float* scratch, float* d_wa, float* d_ba, float* zero, size_t zero_floats, hipStream_t s,
                 bool defer_reduce) {       // defer_reduce: the caller adds the partial sums up later (tr_reduce_pair)
    if (!E) { if (zero_floats) hipMemsetAsync(zero, 0, zero_floats * sizeof(float), s); return; }
    const int nwg = (E + 4 * GATE_EPW - 1) / (4 * GATE_EPW);
    hipLaunchKernelGGL(k_gate_bwd, dim3(nwg), dim3(256), 0, s, E, H, row, pre2, wa, z, attention, dagg, dpre2, scratch, (float4*)zero, zero_floats / 4);
    if (attention && !defer_reduce) hipLaunchKernelGGL(k_partial_reduce, dim3((H + 1 + 63) / 64, min(32, (nwg + 15) / 16)), dim3(256), 0, s, nwg, H, scratch, d_wa, d_ba);
}
// dpre7 from dphi, and d coord_mlp.4.weight
void tr_head_bwd(int E, int H, const float* dphi, const float* w5, const float* pre7, float* dpre7, float* scratch, float* d_w5,
                 float* zero, size_t zero_floats, hipStream_t s, bool defer_reduce, const CoordOutArgs* co) {
    if (!E) { if (zero_floats) hipMemsetAsync(zero, 0, zero_floats * sizeof(float), s); return; }
    const int nwg = (E + 4 * GATE_EPW - 1) / (4 * GATE_EPW);
    hipLaunchKernelGGL(k_head_bwd, dim3(nwg), dim3(256), 0, s, E, H, dphi, w5, pre7, dpre7, scratch, (float4*)zero, zero_floats / 4, co ? *co : CoordOutArgs{});
    if (!defer_reduce) hipLaunchKernelGGL(k_partial_reduce, dim3((H + 63) / 64, min(32, (nwg + 15) / 16)), dim3(256), 0, s, nwg, H, scratch, d_w5, (float*)nullptr);
}
void tr_edge_tail_bwd(int E, int H, const int* row, const int* col, const float* g, const float* d0, const float* Wcol, int ldw,
                      const float4* X, float nc, const float4* dcd, int n_moving, float* dP, float* dQ, float* dWcol, float* dX,
                      float* scratch, hipStream_t s, const float* Wd, float* dd0) {
    if (!E) return;
    const int nwg = (E + 4 * TAIL_EPW - 1) / (4 * TAIL_EPW);
    if (dd0) hipLaunchKernelGGL(k_edge_tail_bwd<true>, dim3(nwg), dim3(256), 0, s, E, H, row, col, g, d0, Wcol, ldw, X, nc, dcd, n_moving,
                                dP, dQ, scratch, dX, Wd, dd0);
    else hipLaunchKernelGGL(k_edge_tail_bwd<false>, dim3(nwg), dim3(256), 0, s, E, H, row, col, g, d0, Wcol, ldw, X, nc, dcd, n_moving,
                            dP, dQ, scratch, dX, (const float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(k_tail_colsum_reduce, dim3((H + 63) / 64, 2, min(32, (nwg + 15) / 16)), dim3(256), 0, s, nwg, H, scratch, dWcol, ldw);
}
// fused: g = (dY W2^T-pack) * SiLU'(pre1) and its whole tail (H = 256; W = split pack of the transposed weight)
void cmdgen_dgrad_tail(int E, const float* dY, const void* Wt, const float* pre1, const int* row, const int* col, const float* d0,
                       const float* Wcol, int ldw, const float4* X, float nc, const float4* dcd, int n_moving, float* dP, float* dQ,
                       float* dWcol, float* dX, float* scratch, int pieces, hipStream_t s, unsigned long long* dbg, bool defer_reduce,
                       const float* Wd, float* dd0) {
    if (E <= 0) return;
    const int nwg = (E + 31) / 32;
    const TailArgs ta{row, col, d0, Wcol, ldw, X, nc, dcd, n_moving, dP, dQ, scratch, dX, dbg, Wd, dd0};
    typedef void (*Kernel)(int, const float*, const void*, const float*, TailArgs);
    static const Kernel tab[2][2] = {{k_dgrad_tail<1>, k_dgrad_tail<3>}, {k_dgrad_tail<1, true>, k_dgrad_tail<3, true>}};     // [input gradients][three pieces]
    hipLaunchKernelGGL(tab[dd0 != nullptr][pieces == 3], dim3(nwg), dim3(256), 0, s, E, dY, Wt, pre1, ta);
    if (!defer_reduce) hipLaunchKernelGGL(k_tail_colsum_reduce, dim3(4, 2, min(32, (nwg + 15) / 16)), dim3(256), 0, s, nwg, 256, scratch, dWcol, ldw);
}
size_t tr_edge_tail_scratch_floats(size_t E, size_t H) { return ((E + 4 * TAIL_EPW - 1) / (4 * TAIL_EPW)) * 2 * H; }
