// cmdgen_train_plan.h - the launch planner of the training step's GEMMs: which weight-gradient kernel runs a group of products, on which grid and
// split-K factor; the k tile, grid and split-K of the plain training GEMM; the rows per tile of the data-gradient kernel.  Pure functions of
// the shapes, the precision and the handle's tuning (TrainTune).  Plain C++17, no HIP: the launchers of kernels_train_gemm.hip and kernels_train_dgrad.hip compute their plan
// and dispatch on it, and tests/train_plan_check.cpp runs the planners on the CPU.
#pragma once

struct TrainTune {              // launch choices of the training step's gradient kernels (cmdgen_set_option; defaults from sweeps on MI355X)
    int wgrad_split = -1;       // weight gradients as three-piece split products: -1 = wherever the handle runs the split engine (tile by wgrad_k128), 0 = never (fp32 instruction), 1 = always on 128 x 128 tiles where the shape allows
    int wgrad_tile = 0;         // 64: never the 128 x 128-tile kernel
    int wgrad_k128 = 131072;    // rows x 128-tiles of a launch from which a three-piece weight gradient uses 128 x 128 tiles (below: 64 x 64)
    int wgrad_split_wgs128 = 384, wgrad_split_wgs64 = 512;   // workgroups the split-K factor of the two split kernels aims at
    int wgrad_wgs = 768;        // ... of the fp32-instruction kernel (3 workgroups of 49 KB LDS per CU; profiles/r02_t3_training_round2.txt)
    int dgrad_mt = 0;           // rows per tile of the data-gradient kernel: 0 = by row count (64 from 24576 rows), 32, 64
    int dgrad_tail = 1;         // 1: dpre of an edge list is consumed inside the second-layer data gradient (k_dgrad_tail)
    int wgrad_stream = 1;       // 1: weight / bias gradients on the handle's second stream, beside the chain of data gradients (cmdgen_train.hip)
};

// ---- split-K: K rows over `zsplit` workgroups per output tile, `kchunk` rows each (partials are combined with atomics) ----
struct SplitK { int kchunk, zsplit; };
// the factor that brings `tiles` output tiles to `target_wgs` workgroups, at most one workgroup per 128 rows
inline int split_k_factor(int tiles, int K, int target_wgs) {
    int z = (target_wgs + tiles - 1) / tiles;
    const int max_split = (K + 127) / 128;
    if (z > max_split) z = max_split;
    return z < 1 ? 1 : z;
}
// a given factor: chunks rounded up to the k tile (kround = 32 or 64), and the workgroups that still have rows
inline SplitK split_k_chunks(int K, int factor, int kround) {
    const int kchunk = ((K + factor - 1) / factor + kround - 1) / kround * kround;
    return SplitK{kchunk, (K + kchunk - 1) / kchunk};
}
inline SplitK plan_split_k(int tiles, int K, int target_wgs, int kround) { return split_k_chunks(K, split_k_factor(tiles, K, target_wgs), kround); }

// ---- weight gradients (cmdgen_wgrad_group) ----
enum class WgradKernel { group, split64, split128 };       // k_wgrad_group (fp32 instruction or bf16 operands, any shape), k_wgrad_split, k_wgrad_split128
struct WgradShape {             // what the choice reads of one product dW[M][N] (+)= dY^T X
    int M = 0, N = 0, lddy_mod4 = 0, ldx_mod4 = 0;
    bool aligned16 = true;      // both operand pointers are 16-byte aligned
    int xs = 0;                 // WgradBatch::xs
};
struct WgradShapes { int n = 0; WgradShape p[8]; };
struct WgradPlan {
    WgradKernel kernel = WgradKernel::group;
    int pieces = 3;             // 1: bf16 operands (the leading piece); 3: fp32-accurate (three pieces; `group`: the fp32 instruction)
    bool xs = false;            // the instantiation that applies SiLU to the X operands marked xs
    int grid[3] = {1, 1, 1};    // (N tiles, M tiles, products x zsplit)
    int kchunk = 0, zsplit = 1;
};
// split3: the handle runs on the split engine, so three-piece (fp32-accurate) weight gradients are allowed; force3: a test asks for them.
// Which kernel (tools/bench_wgrad.py, profiles/r03_n_wgrad.txt; one 256 x 256 product, us per launch):
//     K                fp32 instruction   three pieces 64-tile / 128-tile   bf16 operands 64-tile / 128-tile
//     3 721 (nodes)          18               14 / 17                               12 / 13
//    16 127                  32               32 / 35                               23 / 24
//    36 147                  58               59 / 51                               38 / 37
//   156 316                 253              227 / 175                             155 / 103
// These products are tall and skinny (256 x 256 outputs over 1e4-1e5 rows): operand reads and the split-K atomics bind them, not the
// matrix pipe.  The 128-tile kernel reads each operand row half as often and wins once K >= ~32k (three pieces) / ~64k (bf16).
// The weight gradients run BESIDE the chain of data gradients (cmdgen_train.hip), where the fp32 instruction's long hold on the matrix pipe
// costs the other stream more than its own launch gains: three pieces whenever the handle is on the split engine, 64 x 64 tiles for short
// products and 128 x 128 tiles from  K x (128-tiles of the launch) >= TrainTune::wgrad_k128  (same-box sweeps of that option with both
// streams running: profiles/r05_an, r05_ao).  A 256 x 256 product has four 128-tiles, so with the default 131072 a single product changes
// at K = 131072 / 4 = 32768 rows and a node-level group of four at K = 131072 / 16 = 8192; bf16 operands change at K = 65536 whatever the
// group.  Options: wgrad_split = 0: never three pieces; = 1: always 128 tiles where the shape allows; wgrad_tile = 64: never the 128-tile kernel.
inline WgradPlan plan_wgrad(const WgradShapes& g, int K, bool bf16, bool split3, bool force3, const TrainTune& tune) {
    WgradPlan pl;
    bool ok64 = true, ok128 = tune.wgrad_tile != 64;
    int t64m = 1, t64n = 1, t128m = 1, t128n = 1;         // the grid's tile counts: the largest product's
    long tiles128 = 0;
    for (int p = 0; p < g.n; ++p) {
        const WgradShape& s = g.p[p];
        pl.xs = pl.xs || s.xs != 0;
        ok64 = ok64 && s.M % 64 == 0 && s.N % 64 == 0 && s.lddy_mod4 == 0 && s.ldx_mod4 == 0 && s.aligned16;
        ok128 = ok128 && s.M % 128 == 0 && s.N % 128 == 0;
        if ((s.M + 63) / 64 > t64m) t64m = (s.M + 63) / 64;
        if ((s.N + 63) / 64 > t64n) t64n = (s.N + 63) / 64;
        if (s.M / 128 > t128m) t128m = s.M / 128;
        if (s.N / 128 > t128n) t128n = s.N / 128;
        tiles128 += (long)(s.M / 128) * (s.N / 128);
    }
    ok128 = ok128 && ok64;
    const bool three = !bf16 && (force3 || (split3 && tune.wgrad_split != 0 && ok64));
    const bool sp = ok64 && (bf16 || three);
    const bool sp128 = sp && ok128 && (force3 || tune.wgrad_split == 1 || (bf16 ? K >= 65536 : (long)K * tiles128 >= (long)tune.wgrad_k128));
    pl.pieces = bf16 ? 1 : 3;
    SplitK k;
    if (sp128) {
        pl.kernel = WgradKernel::split128;
        k = plan_split_k((int)tiles128, K, tune.wgrad_split_wgs128, 32);
        pl.grid[0] = t128n; pl.grid[1] = t128m;
    } else {
        pl.kernel = sp ? WgradKernel::split64 : WgradKernel::group;
        k = plan_split_k(t64m * t64n * g.n, K, sp ? tune.wgrad_split_wgs64 : tune.wgrad_wgs, 64);
        pl.grid[0] = t64n; pl.grid[1] = t64m;
    }
    pl.kchunk = k.kchunk; pl.zsplit = k.zsplit; pl.grid[2] = g.n * k.zsplit;
    return pl;
}

// ---- the plain training GEMM (cmdgen_sgemm): C[M][N] = op(A) op(B) on 64 x 64 tiles ----
struct SgemmPlan {
    bool bf16 = false, ta = false, tb = false, a_vec = false, b_vec = false;   // as given: with kt they name the instantiation
    int kt = 64;                // k tile: 64 with few workgroups, 32 from 1024 (see TG_LD)
    int grid[3] = {1, 1, 1};
    int kchunk = 0, z = 1;
    int epi = 0;                // the epilogue actually passed: none with split-K (partials are combined with atomics)
    int slot() const { return (bf16 ? 32 : 0) | (kt == 64 ? 16 : 0) | (ta ? 8 : 0) | (tb ? 4 : 0) | (a_vec ? 2 : 0) | (b_vec ? 1 : 0); }   // index into the launcher's table
};
// split_k: 0 = choose so that the launch fills the chip (aims at 1024 workgroups); 1 = none; > 1: the factor itself
inline SgemmPlan plan_sgemm(bool ta, bool tb, int M, int N, int K, bool a_vec, bool b_vec, int split_k, bool bf16, int epi) {
    SgemmPlan pl;
    pl.bf16 = bf16; pl.ta = ta; pl.tb = tb; pl.a_vec = a_vec; pl.b_vec = b_vec;
    pl.grid[0] = (N + 63) / 64; pl.grid[1] = (M + 63) / 64;
    if (split_k == 0) split_k = split_k_factor(pl.grid[0] * pl.grid[1], K, 1024);
    const SplitK k = split_k > 1 ? split_k_chunks(K, split_k, 64) : SplitK{K, 1};
    pl.kchunk = k.kchunk; pl.z = pl.grid[2] = k.zsplit;
    pl.kt = (long)pl.grid[0] * pl.grid[1] * pl.grid[2] < 1024 ? 64 : 32;
    pl.epi = pl.z > 1 ? 0 : epi;
    return pl;
}

// ---- data gradients (cmdgen_dgrad_split): rows per tile - a test's choice (force_mt: cmdgen_debug_dgrad), the option's, else by row count ----
inline int plan_dgrad(int M, const TrainTune& tune, int force_mt) {
    const bool big = force_mt ? force_mt == 64 : (tune.dgrad_mt ? tune.dgrad_mt == 64 : M >= 24576);
    return big ? 64 : 32;
}
