// cmdgen_coord_proj_body.h - the body of kernels_coord_proj.hip, included once per matrix engine right after cmdgen_node16w_body.h inside the
// same namespace (NW_NPL = 2: half engine, 3: three bf16 pieces): the projection tile uses that file's fragment types, split and MFMA macro,
// so what it multiplies is k_node16w's arithmetic by construction.  No include guard.
#ifndef CP_RD
#define CP_RD 4
#endif
#ifndef CP_NTW
#define CP_NTW 2
#endif
// One projection tile: CP_ROWS rows x (64 CP_NTW) columns of the NEXT block's P (+ b1) or Q from h as the node launch left it.
//   * the weights are the 16-row packs k_node16w reads (WPack::wh16 / ws16 of Wpq_e: 32 n-tiles of 16 columns, P then Q, 8 k-blocks each); a wave
//     owns CP_NTW consecutive n-tiles and keeps a k-block's fragments in registers for both of its 16-row sub-tiles - a tile streams
//     128 KB (half engine, CP_NTW = 2) for 32 rows where the node tile streamed 512 KB of P | Q for 16;
//   * the fragments run CP_RD - 1 k-blocks ahead of the MFMAs in a register ring, the first ones are asked for before the h rows;
//   * every output element sees nw_gemm's products: k ascending, per k-block the pieces in NW_MFMAS' order, fmaf(acc, inv, bias) on the way out.
constexpr int CP_ROWS = 32, CP_NM = CP_ROWS / NW_MT, CP_COLS = 64 * CP_NTW, CP_SLICES = 2 * NW_H / CP_COLS;
static_assert(CP_NTW == 2 || CP_NTW == 4, "a wave owns 32 or 64 output columns");
static_assert(CP_RD >= 2 && CP_RD <= NW_H / 32, "ring depth in k-blocks");

__device__ __forceinline__ void cp_tile_body(float* __restrict__ buf /* [CP_ROWS][NW_LD] */, const Layout& lay, const Work& w, const LayerW& ln,
                                             const int tile, const int slice) {
    constexpr int KB = NW_H / 32;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row0 = tile * CP_ROWS, nvalid = min(CP_ROWS, lay.N - row0);
    const int nt0 = (slice * 4 + wave) * CP_NTW;                               // first n-tile of the wave in [P | Q] (0 .. 31)
    const bool is_p = nt0 < NW_H / 16;
    const int col0 = (nt0 & (NW_H / 16 - 1)) * 16 + (lane & 15);
    const wfrag* wp = reinterpret_cast<const wfrag*>(nw_pack(ln.Wpq_e)) + (size_t)nt0 * KB * KBS + lane;
    wfrag b[CP_RD][CP_NTW][NPL];
#define CP_LOADB(SET, KBLK) _Pragma("unroll") for (int n = 0; n < CP_NTW; ++n) _Pragma("unroll") for (int s = 0; s < NPL; ++s)               \
        b[SET][n][s] = wp[(unsigned)(n * KB + (KBLK)) * KBS + s * 64];
#pragma unroll
    for (int i = 0; i < CP_RD - 1; ++i) { CP_LOADB(i, i) }
    float bias[CP_NTW];
#pragma unroll
    for (int n = 0; n < CP_NTW; ++n) bias[n] = is_p ? ln.b1[col0 + 16 * n] : 0.f;
    const float inv = nw_inv(ln.Wpq_e);
    {   // the h rows of the tile: all global loads in flight together, then the LDS writes (rows past the end: zero)
        float4 hv[CP_ROWS / 4];
#pragma unroll
        for (int j = 0; j < CP_ROWS / 4; ++j) {
            const int r = 4 * j + (tid >> 6);
            hv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < nvalid) hv[j] = reinterpret_cast<const float4*>(w.h + (size_t)(row0 + r) * NW_H)[tid & 63];
        }
#pragma unroll
        for (int j = 0; j < CP_ROWS / 4; ++j) *reinterpret_cast<float4*>(buf + (4 * j + (tid >> 6)) * NW_LD + 4 * (tid & 63)) = hv[j];
    }
    nw_barrier();
    sf32x4 acc[CP_NM][CP_NTW];
#pragma unroll
    for (int m = 0; m < CP_NM; ++m)
#pragma unroll
        for (int n = 0; n < CP_NTW; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[m][n][r] = 0.0f;
    const float* ap = buf + (lane & 15) * NW_LD + (lane >> 4) * 4;            // nw_gemm's A fragment: row lane & 15, k = 4 (lane >> 4) + {0..3, 16..19}
#define CP_MF(M, AI, BS, BI) _Pragma("unroll") for (int n = 0; n < CP_NTW; ++n) acc[M][n] = NW_MFMA(a[AI], b[BS][n][BI], acc[M][n]);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        if (kb + CP_RD - 1 < KB) { CP_LOADB((kb + CP_RD - 1) % CP_RD, kb + CP_RD - 1) }
#pragma unroll
        for (int m = 0; m < CP_NM; ++m) {
            const float* q = ap + m * NW_MT * NW_LD + kb * 32;
            const float4 lo = *reinterpret_cast<const float4*>(q), hi = *reinterpret_cast<const float4*>(q + 16);
            wfrag a[NPL];
            nw_split8(lo, hi, a);
            // (the order of NW_MFMAS in nw_gemm: small terms first)
#if NW_NPL == 3
            CP_MF(m, 2, kb % CP_RD, 0) CP_MF(m, 1, kb % CP_RD, 1) CP_MF(m, 0, kb % CP_RD, 2) CP_MF(m, 1, kb % CP_RD, 0) CP_MF(m, 0, kb % CP_RD, 1) CP_MF(m, 0, kb % CP_RD, 0)
#else
            CP_MF(m, 1, kb % CP_RD, 0) CP_MF(m, 0, kb % CP_RD, 1) CP_MF(m, 0, kb % CP_RD, 0)
#endif
        }
    }
#undef CP_MF
#undef CP_LOADB
    float* __restrict__ out = is_p ? w.P : w.Q;
#pragma unroll
    for (int m = 0; m < CP_NM; ++m)
#pragma unroll
        for (int n = 0; n < CP_NTW; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m * NW_MT + 4 * (lane >> 4) + r;
                if (row < nvalid) out[(size_t)(row0 + row) * NW_H + col0 + 16 * n] = __fmaf_rn(acc[m][n][r], inv, bias[n]);
            }
}

// k_coord_proj: workgroups [0, n_coord) are k_edge_coord<256, 32, false, true, NPL>'s (the same tiles in the same order: xcd_tile walks the list
// with n_coord workgroups); the ones behind them own one projection tile each.  The two roles share nothing inside the launch: h was written by
// the node launch before it, P | Q are read by the message launch after it, the coordinate role reads P_c | Q_c and positions - no flag, no wait.
// Placement: a projection workgroup's column slice is a function of blockIdx.x % 8 alone (workgroups are dealt round-robin over the eight
// XCDs, so the tiles that stream one slice share an L2); the row tile follows from the workgroups of the same residue before it.
__global__ __launch_bounds__(256, 3) void k_coord_proj(Layout lay, Work w, Dims d, LayerW lw, LayerW ln, int layer, int n_coord) {
    union alignas(16) Both { EdgeLds<NW_H, 32, NPL> c; float p[CP_ROWS * NW_LD]; };
    __shared__ Both L;
    static_assert(sizeof(L.p) <= sizeof(L.c.buf), "the projection tile's image fits the coordinate tile's LDS");
    const int bid = (int)blockIdx.x;
    if (bid < n_coord) { edge_coord_body<NW_H, 32, false, true, NPL>(L.c, lay, w, d, lw, layer, TrainSave{}, n_coord); return; }
    constexpr int PER = 8 / CP_SLICES;                                      // XCDs that share a slice
    const int x = bid & 7, first = (n_coord - x + 7) >> 3;                   // first bid >> 3 of this residue behind the coordinate role
    const int tile = ((bid >> 3) - first) * PER + x / CP_SLICES;
    if (tile * CP_ROWS < lay.N) cp_tile_body(L.p, lay, w, ln, tile, x % CP_SLICES);
}
// the grid that gives every (row tile, slice) pair its workgroup under the map above
static int cp_grid(int n_coord, int N) {
    constexpr int PER = 8 / CP_SLICES;
    const int nt = (N + CP_ROWS - 1) / CP_ROWS;
    int grid = n_coord;
    for (int x = 0; x < 8; ++x) {
        const int sub = x / CP_SLICES, cnt = nt > sub ? (nt - sub + PER - 1) / PER : 0, first = (n_coord - x + 7) >> 3;
        if (cnt > 0 && (first + cnt - 1) * 8 + x + 1 > grid) grid = (first + cnt - 1) * 8 + x + 1;
    }
    return grid;
}

// k_coord_readout: the LAST block's coordinate launch (no next block to project for) with the feature part of the readout as its second role
// (LaunchPlan::readout_in_coord).  Workgroups [0, n_coord) are k_edge_coord<256, 32, false, true, NPL>'s, as above; each one behind them owns one
// readout tile of RO_ROWS phar rows (readout_features, cmdgen_egnn_common.h: k_readout's arithmetic by construction).  The roles share nothing: the
// readout role reads h as the last node launch left it and writes columns 3 .. 3 + P of the eps rows; the velocity columns and the NaN flag need
// THIS launch's coordinate sums and are formed by their consumer (k_step_count, k_vel_flag).  The first readout workgroup counts the evaluation
// (ChainState::step: read by embed_body and the step kernels, never by the last block's launches).
struct alignas(16) ReadoutLds { float hrow[RO_ROWS * NW_H]; float wT[NW_H * PLAN_READOUT_DYN_MAX]; ReadoutSmall s; };
__global__ __launch_bounds__(256, 3) void k_coord_readout(Layout lay, Work w, Dims d, LayerW lw, SmallW sw, int layer, int n_coord,
                                                          float* __restrict__ eps_phar, ChainState* chain) {
    union alignas(16) Both { EdgeLds<NW_H, 32, NPL> c; ReadoutLds r; };
    __shared__ Both L;
    static_assert(sizeof(Both) <= 160 * 1024 / 3, "three workgroups per CU, as k_coord_proj");
    const int bid = (int)blockIdx.x;
    if (bid < n_coord) { edge_coord_body<NW_H, 32, false, true, NPL>(L.c, lay, w, d, lw, layer, TrainSave{}, n_coord); return; }
    if (bid == n_coord && threadIdx.x == 0) chain->step += 1;
    readout_features(L.r.hrow, L.r.wT, L.r.s, lay, w, d, sw, eps_phar, nullptr, TrainSave{}, bid - n_coord);
}
