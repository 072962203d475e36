// cmdgen_plan.h - the launch planner: which kernel runs each role of an evaluation (messages, node, coordinates), on which rows per tile,
// grid and matrix engine.  One pure function of the model's dimensions, the layout, the options, the engine and the weight packs that exist.
// Plain C++17, no HIP: cmdgen_api.hip caches its answer in the handle, the launchers switch on it, cmdgen_query reports it, the training
// forward asks for its own mode, and tests/plan_check.cpp runs it on the CPU.
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <string>

enum class PlanEngine { fp32, bf3, half };       // the fp32 matrix instruction; three bf16 pieces per operand; two fp16 pieces (cmdgen_split.h)
inline int plan_mfmas_per_product(PlanEngine e) { return e == PlanEngine::fp32 ? 1 : e == PlanEngine::bf3 ? 6 : 3; }

enum class MsgKernel { tiles, fullk32, e128 };                  // k_edge_msg<H, edge_mt>; its 32-row full-K form; k_edge128<false>
enum class NodeKernel { tiles, node16w, node32p, node64, node64e, node64d };      // tiles: k_node<H, node_mt> (fp32, or register-split on plan.node_eng)
enum class CoordKernel { tiles, fullk32, fullk32_proj, e128 };  // fullk32_proj: k_coord_proj wherever a next block exists (launch_eval: proj_now)

// the packs of one weight matrix that exist (upload_pack: ws / wh always, the 16-row forms where in % 128 == 0)
struct PlanPacks {
    bool ws = false, wh = false, ws16 = false, wh16 = false;
    static PlanPacks of_uploaded(int in) { return PlanPacks{true, true, in % 128 == 0, in % 128 == 0}; }
};

// k_coord_readout stages embedding_out^T [H][dyn] in static LDS beside 8 node rows: with dyn <= 40 the workgroup stays under a third of a CU's 160 KB
constexpr int PLAN_READOUT_DYN_MAX = 40;

struct PlanInput {
    int H = 256, L = 1, S = 1;
    int dyn = 0;                                         // joint_nf + condition_time: the leading dimension of embedding_out^T (0: not known - no readout_in_coord)
    bool joint = false, sin = false, cutoff = true;      // cutoff: a cutoff bounds the radial features
    int n_cus = 256;
    bool gemm_split = true;
    int B = 0;
    const int64_t* nph = nullptr; const int64_t* npk = nullptr;
    int N = 0, Nl = 0, max_n = 0;
    const std::map<std::string, int64_t>* opts = nullptr;        // absent key = unset
    PlanPacks W2, W3, W7, Wpq_e;                                  // before cmdgen_finalize_weights: none
    // training forward (cmdgen_train_forward): the list lengths are known, the packs above are what the step can re-pack
    bool training = false;
    int E = 0, Ec = 0;
    // the k-ascending 16x4 packs of encoder layer 2 and the embedding exist (SmallW::emf_pack: phar_nf 8, joint_nf 32, the time column)
    bool embed_pack = false;

    int64_t opt(const char* key, int64_t dflt) const { if (!opts) return dflt; auto it = opts->find(key); return it == opts->end() ? dflt : it->second; }
    bool opt_set(const char* key) const { return opts && opts->find(key) != opts->end(); }
};

struct LaunchPlan {
    MsgKernel msg = MsgKernel::tiles; NodeKernel node = NodeKernel::tiles; CoordKernel coord = CoordKernel::tiles;
    PlanEngine msg_eng = PlanEngine::fp32, node_eng = PlanEngine::fp32, coord_eng = PlanEngine::fp32;
    int node_mt = 64, edge_mt = 64, coord_mt = 64;       // rows per tile (edge / coord: 128 = the 128-row kernels where they apply)
    int embed_mt = 16;                                   // k_embed's tile inside a conditional chain
    int edge_grid = 512, coord_grid = 256, e128_grid = 512;
    int e128_fused = 3;                                  // bit 0 / 1: the 128-row message / coordinate kernel runs its fused main loop
    int dead_skip = 0, write_embed = 1;
    // what cmdgen_query reports beside the above
    int gemm_split = 1, half_engine = 0, node16_split = 0, node64 = 0, node16w = 1, edge_fullk = 0, proj_in_coord = 0;
    int embed_mfma = 0;                                  // full-path 16-row embedding tiles of phar rows on the fp32 matrix instruction (embed_body)
    int readout_in_coord = 0;                            // the plain sampling chain runs without k_readout: its feature part rides in the last block's coordinate launch (k_coord_readout)
    // training forward
    bool fwd_half = false, node_half = false;            // the two edge kernels / the node kernel run their half save form
    bool reads_frag = false;                             // a tile launch reads the fp32 fragment packs (the generic k_edge_msg / k_node / k_edge_coord forms)
};

inline LaunchPlan make_plan(const PlanInput& in) {
    LaunchPlan p;
    const int n_cus = in.n_cus, H = in.H;
    const bool split = in.gemm_split, sp256 = H == 256 && split;
    // the half engine's operands end at 65504: by default only where the radial features are bounded by a cutoff (every shipped config);
    // 2 forces it, 0 keeps the three-piece bf16 split everywhere
    const int he_opt = (int)in.opt("half_engine", 1);
    const bool half_opt = he_opt == 2 || (he_opt == 1 && in.cutoff);
    const bool half = sp256 && half_opt;                 // the kernels that have a half form are split-engine, H = 256
    p.gemm_split = split ? 1 : 0;
    p.half_engine = split && half_opt ? 1 : 0;

    // Rows per tile: the largest tile that still gives every CU a few workgroups.  Edge counts are only known on
    // the device, so they are estimated from the layout for the geometry a trained model holds and every chain starts
    // from - the phar points inside the pocket (measured on CrossDocked-shaped pockets, bench.py's steady_state_evaluation:
    // C-alpha 9.2 neighbours per node within 6 A and 15 coordinate edges per phar node; full-atom 36 and 54).  A chain of
    // an untrained model drifts to fewer edges; the persistent edge grids just find fewer tiles then.
    double e_est = 0.0, ec_est = 0.0;
    const int64_t N = (int64_t)in.N;
    for (int b = 0; b < in.B; ++b) {
        const double n = (double)(in.nph[b] + in.npk[b]);
        const bool full = !in.cutoff;
        const double deg = full ? n : (n <= 128.0 ? 9.0 : 36.0);
        const double dnode = deg < n ? deg : n;
        double dphar = full ? n : 0.6 * (double)in.nph[b] + (n <= 128.0 ? 0.15 : 0.13) * (double)in.npk[b];   // receivers that move
        if (dphar > n) dphar = n;
        e_est += n * dnode;
        ec_est += in.joint ? n * dnode : (double)in.nph[b] * dphar;                   // joint: every receiver moves
    }
    // thresholds from sweeps on MI355X (fp32 engine: profiles/r01_tile_sweep.txt; split engine:
    // profiles/r02_o_tile_sweep_split.txt, r02_z_tiles_trained_geometry.txt)
    auto pick = [&](double rows) { return rows / 64.0 >= 3.0 * n_cus ? 64 : (rows / 32.0 >= 1.5 * n_cus ? 32 : 16); };
    int node_mt = pick((double)N), edge_mt = pick(e_est), coord_mt = pick(ec_est);
    if (split) {
        // node kernel: 32-row tiles (two LDS images) as soon as they put a workgroup on 0.6 of the CUs (96 C-alpha pockets),
        // never 64 rows; coordinate kernel: 64-row tiles only for very long lists - its list shrinks to a few tiles when a
        // chain drifts, and a lone 64-row tile costs 15 us where a 32-row one costs 10
        node_mt = (double)N / 32.0 >= 0.6 * n_cus ? 32 : 16;
        coord_mt = ec_est / 64.0 >= 6.0 * n_cus ? 64 : (ec_est / 32.0 >= 1.5 * n_cus ? 32 : 16);
    }
    // long lists on the split engine: the 128-row kernels of kernels_edge128.hip (every workgroup owns one chunk of the list; same-box
    // A/B at 256 C-alpha pockets: messages -3 %, coordinate list -14 %; full-atom pockets: level; profiles/r04_d)
    if (sp256) {
        if (e_est / 64.0 >= 4.0 * n_cus) edge_mt = 128;
        // on the half engine the chunked 128-row message kernel wins from ~48 C-alpha pockets (64: 29.6 vs 32.4 us per launch for the 32-row full-K
        // tiles, 96: 37.7 vs 58.7 for the 64-row plane tiles; profiles/r05_t); the coordinate list stays on 32-row tiles until it is long
        if (half && e_est >= 96.0 * n_cus) edge_mt = 128;
        // ... and more 16-row node tiles than CUs means two rounds of k_node16w where 64-row plane tiles need one
        if (half && (N + 15) / 16 > n_cus) node_mt = 32;
        // the 32-row full-K coordinate tiles run on the half engine, 16-row tiles on the fp32 instruction: 32 rows from a quarter of a tile per CU
        // (48 pockets: 32.9 us per launch on 16-row tiles, 64 pockets: 18.3 on 32-row ones)
        if (half && coord_mt == 16 && ec_est / 32.0 >= 0.25 * n_cus) coord_mt = 32;
        if (half && edge_mt == 16 && e_est / 32.0 >= 0.25 * n_cus) edge_mt = 32;        // (16 pockets: 29.0 us on 16-row tiles; 32 pockets: 21.2 on 32-row ones)
        if (ec_est / 32.0 >= 3.0 * n_cus) coord_mt = 128;      // (from 128 C-alpha pockets: profiles/r04_h)
        // dense samples (full-atom pockets: 36 neighbours per node, ~60 coordinate edges per phar point while the points sit at the pocket centre):
        // a receiver's edges outnumber the rows of a 16- / 32-row tile, its sum would be three or more float-atomic partials whose order the
        // hardware picks - the 128-row kernels (variable tiles, >= 128-row chunks) keep it at two, so full-atom chains are reproducible run to run
        if (in.max_n > 128) { edge_mt = 128; coord_mt = 128; }
        // joint chains noise the pocket nodes too: over the first steps a C-alpha sample is nearly fully connected (~48 k edges per evaluation
        // on average at 64 pockets where the layout estimate says 34 k), and over those lists the 32-row full-K message tiles win - same-box
        // chains at 64 / 128 / 256 pockets: +8.6 / +5.0 / +4.7 % (profiles/r06_m); the coordinate list (the same edges) stays on 128 rows
        else if (half && in.joint && edge_mt == 128) edge_mt = 32;
    }
    // (the fp32 instruction / other widths have no 128-row kernels: their largest tile keeps most dense receivers at two partials)
    if (!sp256 && in.max_n > 128) { edge_mt = 64; coord_mt = 64; }
    node_mt = (int)in.opt("node_mt", node_mt);
    edge_mt = (int)in.opt("edge_mt", edge_mt);
    coord_mt = (int)in.opt("coord_mt", coord_mt);
    // grids of the persistent-style edge kernels: enough workgroups for the estimated tile count, capped at
    // what is co-resident per CU (2 at 64-row tiles, 4 below); surplus tiles are picked up by the loop
    auto grid_for = [&](double rows, int mt) {
        const double tiles = rows / mt + 1.0;
        const int cap = (mt >= 64 ? 2 : 4) * n_cus;
        int g = (int)(tiles * 1.25) + 8;
        return g < n_cus / 4 ? n_cus / 4 : (g > cap ? cap : g);
    };
    p.edge_grid = grid_for(e_est, edge_mt);
    p.coord_grid = grid_for(ec_est, coord_mt);
    // the 128-row kernels' fused main loop pays once a workgroup (two per CU) walks more than one tile: same-box chains, profiles/r06_f
    // (64 C-alpha pockets, one 96-row tile per workgroup: -1.6 %; 96 pockets, one 128-row tile: +1.2 %; 128 pockets: +2 %; 256: +3 %; full-atom: +8 %)
    p.e128_fused = (e_est > 160.0 * n_cus ? 1 : 0) | (ec_est > 160.0 * n_cus ? 2 : 0);
    if (in.opt_set("e128_fused")) p.e128_fused = (int)in.opt("e128_fused", 3) & 3;
    if (in.opt_set("edge_wgs_per_cu")) p.edge_grid = (int)in.opt("edge_wgs_per_cu", 2) * n_cus;
    if (in.opt_set("coord_wgs_per_cu")) p.coord_grid = (int)in.opt("coord_wgs_per_cu", 2) * n_cus;
    if (node_mt != 64 && node_mt != 32 && node_mt != 16) node_mt = 64;
    for (int* m : {&edge_mt, &coord_mt}) if (*m != 128 && *m != 64 && *m != 32 && *m != 16) *m = 64;     // 128: kernels_edge128.hip
    if (!sp256) { if (edge_mt == 128) edge_mt = 64; if (coord_mt == 128) coord_mt = 64; }      // the 128-row kernels are split-engine, H = 256
    if (in.sin && H == 512) { if (edge_mt > 32) edge_mt = 32; if (coord_mt > 32) coord_mt = 32; }   // (64-row tiles + the 55 KB of feature columns exceed the LDS)
    p.edge_fullk = (sp256 && in.opt("edge_fullk", 1) != 0) ? 1 : 0;
    {
        const int wgs = (int)in.opt("e128_wgs_per_cu", 2);
        p.e128_grid = (wgs >= 1 && wgs <= 4 ? wgs : 2) * n_cus;
    }
    p.write_embed = in.opt("write_embed", 1) != 0 ? 1 : 0;
    {   // k_node64 (kernels_node64.hip: 64-row node tiles, the A operand as producer-side bf16 planes, one workgroup per CU) against
        // k_node<H, 32> (register split, two workgroups per CU).  Per launch the 64-row kernel takes ~0.89 of a co-resident pair of
        // 32-row tiles, a 32-row tile alone on its CU ~0.62 of that 64-row tile (profiles/r03_m_node64.txt), so the choice is a matter
        // of how the tiles fill the CUs: compare the rounds each needs.  Option "node64" = 0 / 1 (/ 32: the 32-row planes tile) overrides.
        int on = 0;
        if (sp256 && n_cus > 0) {
            const int ncu = n_cus, t64 = (in.N + 63) / 64, t32 = (in.N + 31) / 32;
            const float cost64 = (float)((t64 + ncu - 1) / ncu);
            const int full = t32 / (2 * ncu), rem = t32 - full * 2 * ncu;
            float cost32 = 1.12f * full + (rem == 0 ? 0.f : rem <= ncu ? 0.62f : 1.12f);
            // half engine: k_node64 has a half form, the register-split 32-row tile has not - measured per launch (profiles/r05_t) 54.0 vs 44.6 us at
            // 96 pockets (177 32-row tiles, one per CU), 87.5 vs 46.1 at 160 (two per CU)
            if (half) cost32 = 1.9f * full + (rem == 0 ? 0.f : rem <= ncu ? 1.22f : 1.9f);
            on = cost64 < cost32 && !(half && node_mt == 16);
            // Round 6: on the half engine the 32-ROW plane tile (k_node32p: 193 registers, 67 KB of LDS - TWO workgroups per CU, so one's HBM phases run
            // beside the other's GEMMs) beats both the 64-row tile and the register-split 32-row tile wherever the eight-wave 16-row tile does not apply:
            // per evaluation -13 % at 80 C-alpha pockets, -10 % at 128, -1.4 % at 256, -2 % / -1.4 % at 64 / 256 full-atom pockets
            // (profiles/r06_h_node_tile_sweep.txt; the 64-row tile stays behind option node64 = 1)
            if (half && node_mt != 16) on = 32;
            // ... except where the 32-row tiles need both slots of a CU and the 64-row tiles still fit one per CU (8 k < N <= 16 k rows on 256 CUs: 144 - 272
            // C-alpha pockets, the north star's 256): there the 64-row tile on EIGHT waves (k_node64e) streams the weights once per CU instead of twice and its
            // GEMM phases run at the matrix pipe's rate (k_node32p's are bound by the 64 B/clk of L1 fill: 85 B/clk asked) - per evaluation -1.4 .. -1.9 %
            // (profiles/r06_n_node64e.txt)
            if (on == 32 && t32 > ncu && t64 <= ncu) on = 8;
            // ... and with more 64-row tiles than CUs the lean 64-row tile, two workgroups per CU (k_node64d: 43 B/clk of weight fragments asked, and a
            // partner workgroup beside every phase): per launch -5 % at 288 C-alpha pockets, -8 % at 384, -15 % at 512, -7 % / -11 % at 64 / 128 full-atom pockets
            else if (on == 32 && t64 > ncu) on = 2;
            if (in.opt_set("node64")) { const int64_t v = in.opt("node64", 0); on = v == 32 ? 32 : v == 8 ? 8 : v == 2 ? 2 : v != 0; }
        }
        p.node64 = on;
        p.dead_skip = (in.joint || in.S != 1) ? 0 : (int)in.opt("dead_skip", 2);   // (hop levels count blocks of ONE GCL)      // 2 (default): every block by hop level; 1: the last block only; 0: off
    }
    // 16-row node tiles on the split engine too (v_mfma_f32_16x16x32_bf16; H >= 128): k_node<256,16> 35.0 -> 31.4 us at B=64 -
    // bound by the 6 B/weight stream of one workgroup per 16 rows, not by the matrix pipe (profiles/r03_b_*); option "node16_split" = 0 opts out
    p.node16_split = (split && H >= 128 && in.opt("node16_split", 1) != 0) ? 1 : 0;
    p.node16w = in.opt("node16w", 1) != 0 ? 1 : 0;
    {   // k_embed: inside a conditional chain only the phar tiles take the full path (the pocket rows come from the per-chain
        // cache), and they are few: 16-row tiles spread them over twice the CUs and halve the two projection passes of each
        // (B=256: 120 tiles of 32 rows 38.6 us -> 240 tiles of 16 rows)
        p.embed_mt = (int)in.opt("embed_mt", (((double)in.Nl / 16.0 <= 2.0 * n_cus && !in.joint) ? 16 : node_mt));
        if (p.embed_mt != 16 && p.embed_mt != 32 && p.embed_mt != 64) p.embed_mt = node_mt;
    }
    // the full-path 16-row tile of phar rows with encoder layer 2 and the embedding as v_mfma_f32_16x16x4_f32 chains (k ascending from the bias: the
    // scalar form's bits) and every operand requested at kernel start: H = 256, a 16-row tile (k_write_embed's pairs inside a chain, k_embed<256, 16>),
    // never the training forward.  Option "embed_mfma": 0 never, 1 wherever that holds, unset: where it measured faster in every run - from 30 full-path
    // tiles (32, 64 and 256 C-alpha pockets of 15 points; at 20 pockets of 3 points, four tiles, the rates overlap: profiles/phar_tiles_ab.txt).
    p.embed_mfma = H == 256 && in.embed_pack && !in.training && (p.embed_mt == 16 || node_mt == 16) && in.opt("embed_mfma", in.Nl >= 30 * 16 ? 1 : 0) != 0 ? 1 : 0;
    // (the node kernel avoids its 64-row register-split tiles on the split engine: 87 vs 132 us at B=256, profiles/r02_o_tile_sweep_split.txt)
    if (split && node_mt == 64 && !in.opt_set("node_mt")) node_mt = 32;
    p.node_mt = node_mt; p.edge_mt = edge_mt; p.coord_mt = coord_mt;

    const PlanEngine tiles32 = split ? PlanEngine::bf3 : PlanEngine::fp32;      // the generic tiles of >= 32 rows; 16-row edge tiles are always fp32 MFMA
    if (in.training) {
        // The forward pass of a training step is the sampler's evaluation with save hooks.  Its two edge kernels run on the half engine (two fp16
        // pieces, three MFMAs per product: cmdgen_split.h) wherever the sampler would use it ...
        const int train_half = (int)in.opt("train_half", 1);
        p.fwd_half = sp256 && half_opt && p.edge_fullk && in.W2.wh && train_half != 0;
        // ... and the node kernel as the sampler's eight-wave 16-row tile (k_node16w)
        // (option train_node16: 16-row tiles for the node kernel at EVERY size - the save-hook form of the node kernel exists on the half engine
        // for these tiles only; larger layouts otherwise fall back to the fp32-instruction k_node<H, 32 / 64, SAVE>)
        if (p.fwd_half && in.opt("train_node16", 1) != 0) p.node_mt = 16;
        p.node_half = p.fwd_half && p.node_mt == 16 && in.W3.wh16 && train_half != 2;
        p.dead_skip = 0; p.node64 = 0; p.proj_in_coord = 0;              // the training forward skips nothing, and the plane kernels have no save form
        // tile rows of the two edge kernels: the training forward knows its lists' lengths (the sampler estimates them, and its
        // 128-row kernels have no activation-saving form): 32-row tiles until 64-row ones fill every CU four times over
        auto rows = [&](int n) { return n / 64 >= 4 * n_cus ? 64 : (n / 32 >= n_cus / 4 ? 32 : 16); };
        auto grid = [&](int n, int mt) { const int cap = (mt >= 64 ? 2 : 4) * n_cus, g = (int)((n / mt + 1) * 1.25) + 8; return g < n_cus / 4 ? n_cus / 4 : (g > cap ? cap : g); };
        if (!in.opt_set("edge_mt") || p.edge_mt == 128) { p.edge_mt = rows(in.E); p.edge_grid = grid(in.E, p.edge_mt); }
        if (!in.opt_set("coord_mt") || p.coord_mt == 128) { p.coord_mt = rows(in.Ec); p.coord_grid = grid(in.Ec, p.coord_mt); }
        if (p.fwd_half) {     // the half form exists for 32-row full-K tiles (three workgroups per CU)
            p.edge_mt = 32; p.edge_grid = grid(in.E, 32); p.coord_mt = 32; p.coord_grid = grid(in.Ec, 32);
        }
        // the generic save forms multiply on the split engine only where the step re-packs split weights (H = 256: edge_mlp.2 / coord_mlp.2)
        const PlanEngine save32 = split && H == 256 && in.W2.ws ? PlanEngine::bf3 : PlanEngine::fp32;
        p.msg = p.fwd_half ? MsgKernel::fullk32 : MsgKernel::tiles;
        p.msg_eng = p.fwd_half ? PlanEngine::half : (p.edge_mt >= 32 ? save32 : PlanEngine::fp32);
        p.coord = p.fwd_half ? CoordKernel::fullk32 : CoordKernel::tiles;
        p.coord_eng = p.fwd_half ? PlanEngine::half : (p.coord_mt >= 32 ? save32 : PlanEngine::fp32);
        p.node = p.node_half && H == 256 ? NodeKernel::node16w : NodeKernel::tiles;        // (k_node's save form is the fp32 instruction)
        p.node_eng = p.node == NodeKernel::node16w ? PlanEngine::half : PlanEngine::fp32;
        p.reads_frag = p.msg == MsgKernel::tiles || p.coord == CoordKernel::tiles || p.node == NodeKernel::tiles;
        return p;
    }

    // messages: the 128-row kernel, then the 32-row full-K tiles, then the generic tiles
    if (edge_mt == 128 && in.W2.ws) { p.msg = MsgKernel::e128; p.msg_eng = half && in.W2.wh ? PlanEngine::half : PlanEngine::bf3; }
    else if (p.edge_fullk && edge_mt == 32) { p.msg = MsgKernel::fullk32; p.msg_eng = half && in.W2.wh ? PlanEngine::half : PlanEngine::bf3; }
    else { p.msg = MsgKernel::tiles; p.msg_eng = edge_mt >= 32 ? tiles32 : PlanEngine::fp32; }
    // node: the plane kernels (k_node64 and its kin), then the eight-wave 16-row tile, then the generic tiles
    if (p.node64 && in.W3.ws) {
        p.node_eng = half && in.W3.wh ? PlanEngine::half : PlanEngine::bf3;
        const bool eight = p.node_eng == PlanEngine::half;             // k_node64d / k_node64e exist on the half engine
        p.node = p.node64 == 2 && eight ? NodeKernel::node64d : p.node64 == 8 && eight ? NodeKernel::node64e : p.node64 == 32 ? NodeKernel::node32p : NodeKernel::node64;
    } else if (H == 256 && node_mt == 16 && p.node16_split && p.node16w && in.W3.ws16) {
        p.node = NodeKernel::node16w; p.node_eng = half && in.W3.wh16 ? PlanEngine::half : PlanEngine::bf3;
    } else {
        p.node = NodeKernel::tiles;
        p.node_eng = node_mt >= 32 ? tiles32 : (p.node16_split && in.W3.ws16 ? PlanEngine::bf3 : PlanEngine::fp32);
    }
    // coordinates: as the messages
    if (coord_mt == 128 && in.W7.ws) { p.coord = CoordKernel::e128; p.coord_eng = half && in.W7.wh ? PlanEngine::half : PlanEngine::bf3; }
    else if (p.edge_fullk && coord_mt == 32) { p.coord = CoordKernel::fullk32; p.coord_eng = half && in.W7.wh ? PlanEngine::half : PlanEngine::bf3; }
    else { p.coord = CoordKernel::tiles; p.coord_eng = coord_mt >= 32 ? tiles32 : PlanEngine::fp32; }
    p.reads_frag = p.msg == MsgKernel::tiles || p.coord == CoordKernel::tiles || p.node == NodeKernel::tiles;
    // the next block's P | Q projections as column-sliced tiles inside the coordinate launch (kernels_coord_proj.hip) instead of in k_node16w,
    // whose 16-row tile streams every weight it multiplies: only where k_node16w takes the node launches AND the coordinate list runs on the
    // 32-row full-K tile (the launch the projection tiles join), one GCL per block, the conditional model, and both roles on the same engine.
    // Option "proj_in_coord": 0 never, 1 wherever that holds, unset: where it measured faster (profiles/proj_in_coord_ab.txt).
    const bool can = p.node == NodeKernel::node16w && p.coord == CoordKernel::fullk32 && in.S == 1 && in.L > 1 && !in.joint && p.node_eng == p.coord_eng &&
                     (p.node_eng == PlanEngine::half ? in.Wpq_e.wh16 : in.Wpq_e.ws16);
    p.proj_in_coord = can && in.opt("proj_in_coord", 1) != 0 ? 1 : 0;
    if (p.proj_in_coord) p.coord = CoordKernel::fullk32_proj;
    // k_readout's feature part (embedding_out + the decoders of the phar rows) as tiles behind the LAST block's coordinate launch, the velocity and the
    // batch-global NaN flag formed by their consumer (k_step_count, k_vel_flag): one launch less per step of the plain conditional sampling chain
    // (launch_eval / readout_mode hold the per-evaluation conditions).  Only where that launch is the 32-row full-K tile (three workgroups per CU, mostly
    // idle CUs), one GCL per block, the conditional model, samples the per-sample kernels run on four waves.
    // Option "readout_in_coord": 0 never, 1 wherever that holds, unset: where it measured faster (profiles/readout_in_coord_ab.txt).
    const bool can_ro = H == 256 && !in.joint && in.S == 1 && (p.coord == CoordKernel::fullk32 || p.coord == CoordKernel::fullk32_proj) &&
                        in.dyn >= 1 && in.dyn <= PLAN_READOUT_DYN_MAX && in.max_n <= 128;
    p.readout_in_coord = can_ro && in.opt("readout_in_coord", 1) != 0 ? 1 : 0;
    return p;
}

// The dynamic LDS of a derived chain's step kernel (StepWg, cmdgen_step_parts.h): a float4 position and a degree per node of the largest sample, z per row.
inline size_t plan_step_lds(int max_n, int P) { return (size_t)max_n * (16 + sizeof(int) + (size_t)(3 + P) * sizeof(float)); }

// The restrained chain's step kernel (k_restrained_step_count, kernels_restrain.hip) runs in the plain chain's place and takes both of its forms: where
// readout_in_coord holds it forms the velocity and the NaN flag itself (readout_mode).  Beside k_step_count's LDS (a float4 position and a degree per node,
// z and the velocity per row) it keeps the denoised estimate, the displacement and the energy term of every row: bytes per workgroup, at most 64 KiB.
constexpr size_t PLAN_RESTRAINED_LDS_MAX = 64 * 1024;
inline size_t plan_restrained_step_lds(int max_n, int P) { return plan_step_lds(max_n, P) + (size_t)max_n * (3 + 7) * sizeof(float); }

// The restrained edit chain's step kernel (k_restrained_edit_step_count, kernels_restrain.hip) keeps k_inpaint_step_count's LDS (a float4 position and a
// degree per node, z per row), then the denoised estimate, the displacement and the energy term of every row; eps comes from eps_tmp, so there is no
// velocity array.  Bytes per workgroup, at most PLAN_RESTRAINED_LDS_MAX.
inline size_t plan_restrained_edit_step_lds(int max_n, int P) { return plan_step_lds(max_n, P) + (size_t)max_n * 7 * sizeof(float); }

// The restrained diverse chain's step kernel (k_diverse_restrained_step_count, kernels_restrain.hip) keeps the same: the plain step's LDS, then the
// denoised estimate, the restraint displacement and the energy term of every row (the overlap displacement comes from global memory).  92 B per node at
// phar_nf 8: bytes per workgroup, at most PLAN_RESTRAINED_LDS_MAX - 712 nodes, where the diverse chain alone takes 1024.
inline size_t plan_diverse_restrained_step_lds(int max_n, int P) { return plan_step_lds(max_n, P) + (size_t)max_n * 7 * sizeof(float); }

// The diverse chain (kernels_diverse.hip): its step kernel keeps plan_step_lds; k_diverse_frame keeps a float4 per pocket atom of the largest sample
// (less, so the step's check covers it); k_diverse_pair's LDS is static.
inline size_t plan_diverse_frame_lds(int max_n) { return (size_t)max_n * 16; }

// the launch keys of cmdgen_query (include/cmdgen_hip.h); false: not a launch key
inline bool plan_query(const LaunchPlan& p, const char* key, int64_t* value) {
    const struct { const char* key; int64_t v; } keys[] = {
        {"node_mt", p.node_mt}, {"edge_mt", p.edge_mt}, {"coord_mt", p.coord_mt}, {"edge_grid", p.edge_grid}, {"coord_grid", p.coord_grid},
        {"e128_fused", p.e128_fused}, {"gemm_split", p.gemm_split}, {"half_engine", p.half_engine}, {"node16_split", p.node16_split},
        {"node64", p.node64}, {"node16w", p.node16w}, {"proj_in_coord", p.proj_in_coord}, {"edge_fullk", p.edge_fullk}, {"dead_skip", p.dead_skip},
        {"embed_mfma", p.embed_mfma}, {"readout_in_coord", p.readout_in_coord},
        {"msg_mfmas_per_product", plan_mfmas_per_product(p.msg_eng)}, {"node_mfmas_per_product", plan_mfmas_per_product(p.node_eng)},
        {"coord_mfmas_per_product", plan_mfmas_per_product(p.coord_eng)}};
    for (const auto& k : keys) if (strcmp(k.key, key) == 0) { *value = k.v; return true; }
    return false;
}
