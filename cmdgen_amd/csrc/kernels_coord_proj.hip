// kernels_coord_proj.hip - k_coord_proj: the coordinate update of block l on 32-row full-K tiles (edge_coord_body, kernels_egnn_coord.hip) and the
// edge-MLP projections P | Q of block l + 1 in ONE launch (conditional sampler, H = 256, small batches).
//
// Why.  k_node16w (kernels_node16w.hip) multiplies 16 rows per workgroup and streams every weight of its chain of GEMMs for them: 1.8 MB per tile
// on the half engine, 236 tiles at 64 C-alpha pockets, ~425 MB per launch out of the L2s - that stream, at what the chip's L2s deliver to one
// workgroup per CU, IS the launch's time.  Two of the tile's six weight units are the NEXT block's P | Q, which nothing in the
// node tile reads.  Here they run as independent tiles of 32 rows x 128 columns (a quarter of one projection's weights for twice the rows) beside
// the coordinate launch, which at this size is the latency chain of a few tiles on mostly idle CUs.  No exchange between workgroups: both roles
// read what earlier launches wrote.  Every P / Q element sees the MFMAs nw_gemm gave it, in the same order (cmdgen_coord_proj_body.h).
//
// k_coord_readout: the LAST block's coordinate launch has no next block to project for; in the plain sampling chain its second role is the feature
// part of k_readout (embedding_out + the decoders of the phar rows), which depends on the last node launch alone - one launch less per step.
#define CMDGEN_H_PART 2                 // edge_coord_body and its helpers only, no launchers
#include "kernels_egnn_coord.hip"
#include "cmdgen_split.h"

#define NW_NPL 2
namespace cp_half {
#include "cmdgen_node16w_body.h"
#include "cmdgen_coord_proj_body.h"
}
#undef NW_NPL
#undef NW_MFMA
#define NW_NPL 3
namespace cp_bf3 {
#include "cmdgen_node16w_body.h"
#include "cmdgen_coord_proj_body.h"
}
#undef NW_NPL
#undef NW_MFMA

// launcher of the merged kernel (CoordKernel::fullk32_proj, for a block that has a next one in an evaluation with EvalLaunch::proj_now: this
// evaluation's k_node16w launches leave the next block's P | Q out - the planner and launch_eval hold the conditions)
void cmdgen_launch_coord_proj(const EvalLaunch& a, int l, hipStream_t s) {
    const LayerW& lw = a.layers[unit_of(a, l)];
    const LayerW& ln = a.layers[unit_of(a, l) + 1];
    const int cg = a.plan.coord_grid;
    if (a.plan.coord_eng == PlanEngine::half) {
        const int grid = cp_half::cp_grid(cg, a.lay.N);
        if (a.pe_start) hipExtLaunchKernelGGL(cp_half::k_coord_proj, dim3(grid), dim3(256), 0, s, a.pe_start, a.pe_stop, 0, a.lay, a.w, a.d, lw, ln, l, cg);
        else hipLaunchKernelGGL(cp_half::k_coord_proj, dim3(grid), dim3(256), 0, s, a.lay, a.w, a.d, lw, ln, l, cg);
    } else {
        const int grid = cp_bf3::cp_grid(cg, a.lay.N);
        if (a.pe_start) hipExtLaunchKernelGGL(cp_bf3::k_coord_proj, dim3(grid), dim3(256), 0, s, a.pe_start, a.pe_stop, 0, a.lay, a.w, a.d, lw, ln, l, cg);
        else hipLaunchKernelGGL(cp_bf3::k_coord_proj, dim3(grid), dim3(256), 0, s, a.lay, a.w, a.d, lw, ln, l, cg);
    }
}

// launcher of the last block's coordinate launch with the readout tiles behind it (EvalLaunch::readout_now; the planner holds the conditions:
// H = 256, the 32-row full-K coordinate tile, dyn <= PLAN_READOUT_DYN_MAX)
void cmdgen_launch_coord_readout(const EvalLaunch& a, int l, float* eps_phar, ChainState* chain, hipStream_t s) {
    const LayerW& lw = a.layers[unit_of(a, l)];
    const int cg = a.plan.coord_grid, grid = cg + (a.lay.Nl + RO_ROWS - 1) / RO_ROWS;
    if (a.plan.coord_eng == PlanEngine::half) {
        if (a.pe_start) hipExtLaunchKernelGGL(cp_half::k_coord_readout, dim3(grid), dim3(256), 0, s, a.pe_start, a.pe_stop, 0, a.lay, a.w, a.d, lw, a.sw, l, cg, eps_phar, chain);
        else hipLaunchKernelGGL(cp_half::k_coord_readout, dim3(grid), dim3(256), 0, s, a.lay, a.w, a.d, lw, a.sw, l, cg, eps_phar, chain);
    } else {
        if (a.pe_start) hipExtLaunchKernelGGL(cp_bf3::k_coord_readout, dim3(grid), dim3(256), 0, s, a.pe_start, a.pe_stop, 0, a.lay, a.w, a.d, lw, a.sw, l, cg, eps_phar, chain);
        else hipLaunchKernelGGL(cp_bf3::k_coord_readout, dim3(grid), dim3(256), 0, s, a.lay, a.w, a.d, lw, a.sw, l, cg, eps_phar, chain);
    }
}
