// cmdgen_launch.h - the launchers of the evaluation and of the chains: every function one translation unit defines and another
// calls, declared once.  The calling file AND the defining file include this header, so a changed signature is a compile error
// instead of an unresolved (or, with default arguments, a silently different) call.  Declarations only: nothing here beyond
// cmdgen_dev.h's types.
#pragma once
#include "cmdgen_dev.h"

// kernels_egnn.hip: one evaluation (radius graph, k_embed, per block the message / node / coordinate launches, k_readout)
void cmdgen_launch_eval(const EvalLaunch& a, const float* xh_phar, const float* xh_pocket, const float* t_arr, const float4* coef,
                        ChainState* chain, float* eps_phar, float* eps_pocket, hipStream_t s, hipEvent_t* ev);
void cmdgen_launch_nan_fix(const EvalLaunch& a, float* eps_phar, hipStream_t s);
void cmdgen_launch_vel_flag(const EvalLaunch& a, float* eps_phar, hipStream_t s);     // velocity columns + NaN flag alone, in front of the decode (readout_mode)
void cmdgen_launch_save_positions(const EvalLaunch& a, float4* X, hipStream_t s);
void cmdgen_readout_allow_lds(size_t bytes);            // k_readout's dynamic LDS above the 64 KiB default (hidden_nf 512)

// kernels_egnn_graph.hip: radius graph + k_embed
void cmdgen_launch_edges(const EvalLaunch& a, const float* xh_phar, const float* xh_pocket, hipStream_t s);
void cmdgen_build_pocket_cache(const EvalLaunch& a, const float* xh_phar, const float* xh_pocket, const float* t01,
                               float* c, float* P0, float* Q0, float* dh, float* dP, float* dQ, hipStream_t s);
void cmdgen_edge_kernels_allow_lds(size_t bytes);       // hipFuncSetAttribute above the 64 KiB default
void cmdgen_launch_edge_count(const EvalLaunch& a, const float* xh_phar, const float* xh_pocket, hipStream_t s);
void cmdgen_launch_edge_write(const EvalLaunch& a, const float* x0_from /* null, or the phar rows pass 2 copies into X0 (readout_mode) */, hipStream_t s);

// per-family launch entry points (each picks the instantiation for a.d.H and the launch's tile rows); the *_hx forms are the same
// families at the hidden sizes other than 256, built as translation units of their own (kernels_egnn_*_hx.hip, CMDGEN_H_PART)
void cmdgen_launch_embed_tiles(const EvalLaunch& a, int mt, const float* xp, const float* xq, const float* t, const float4* coef, ChainState* chain, hipStream_t s);
void cmdgen_launch_embed_tiles_hx(const EvalLaunch& a, int mt, const float* xp, const float* xq, const float* t, const float4* coef, ChainState* chain, hipStream_t s);
void cmdgen_launch_write_embed_tiles(const EvalLaunch& a, int mt, const float* xp, const float* xq, const float* t, const float4* coef, ChainState* chain, hipStream_t s);   // H = 256
void cmdgen_embed_only_hx(const EvalLaunch& a, const float* xp, const float* xq, const float* t, hipStream_t s);
void cmdgen_launch_msg_tiles(const EvalLaunch& a, int l, hipStream_t s);                   // kernels_egnn_msg.hip: the generic tiles
void cmdgen_launch_msg_tiles_hx(const EvalLaunch& a, int l, hipStream_t s);
void cmdgen_launch_msg_fullk(const EvalLaunch& a, int l, hipStream_t s);                   // ... and the 32-row full-K tiles (H = 256)
void cmdgen_launch_edge_msg_only(const EvalLaunch& a, int layer, hipStream_t s);           // kernels_egnn.hip: one block's message launch alone
void cmdgen_launch_node_tiles(const EvalLaunch& a, int l, hipStream_t s);                  // kernels_egnn_node.hip
void cmdgen_launch_node_tiles_hx(const EvalLaunch& a, int l, hipStream_t s);
void cmdgen_launch_coord_tiles(const EvalLaunch& a, int l, hipStream_t s);                 // kernels_egnn_coord.hip: the generic tiles
void cmdgen_launch_coord_tiles_hx(const EvalLaunch& a, int l, hipStream_t s);
void cmdgen_launch_coord_fullk(const EvalLaunch& a, int l, hipStream_t s);                 // ... and the 32-row full-K tiles (H = 256)
// one kernel family each, picked by launch_eval's switches on EvalLaunch::plan (kernels_egnn.hip)
void cmdgen_launch_node64(const EvalLaunch& a, int l, hipStream_t s);         // kernels_node64.hip: k_node for large batches
void cmdgen_launch_node16w(const EvalLaunch& a, int l, hipStream_t s);        // kernels_node16w.hip: 16-row tiles on eight waves (small batches)
void cmdgen_launch_msg128(const EvalLaunch& a, int l, hipStream_t s);         // kernels_edge128.hip: the edge kernels for long lists (128-row tiles)
void cmdgen_launch_coord128(const EvalLaunch& a, int l, hipStream_t s);
void cmdgen_launch_coord_proj(const EvalLaunch& a, int l, hipStream_t s);     // kernels_coord_proj.hip: the 32-row full-K coordinate tiles + the next block's P | Q tiles in one launch (EvalLaunch::proj_now)

void cmdgen_launch_coord_readout(const EvalLaunch& a, int l, float* eps_phar, ChainState* chain, hipStream_t s);   // ... the same tiles + the readout's feature tiles: the LAST block (EvalLaunch::readout_now)

// kernels_ddpm.hip: the conditional chain
void cmdgen_launch_chain_init(const Layout& lay, const Dims& d, const ChainBuf& c, const float* px, const float* poh, hipStream_t s);
void cmdgen_launch_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const Work& w, const float* eps, int own_vel /* readout_mode */, hipStream_t s);
void cmdgen_launch_chain_final(const Layout& lay, const Dims& d, const ChainBuf& c, const Work& w, const float* eps, float* xo, float* po,
                               unsigned int* cog, hipStream_t s);
void cmdgen_launch_debug_noise(unsigned long long seed, long long pocket_id, int draw, int n_nodes, int width, float* out, hipStream_t s);

// kernels_restrain.hip: the restrained chain (the conditional chain with a guidance term in the mean of every posterior op)
void cmdgen_launch_restrain_prep(const Layout& lay, const Dims& d, const RestrainBuf& rb, const float* px, hipStream_t s);
void cmdgen_launch_restrained_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const RestrainBuf& rb, const Work& w,
                                         const float* eps, int own_vel /* readout_mode */, hipStream_t s);
void cmdgen_launch_restrained_edit_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const InpaintBuf& ip, const RestrainBuf& rb,
                                              const Work& w, const float* eps, hipStream_t s);   // the edit chain's op with the guidance in op A
void cmdgen_launch_restrain_energy(const Layout& lay, const Dims& d, const RestrainBuf& rb, const float* xo, const float* po,
                                   float* energy_out, hipStream_t s);
// ... and the restrained diverse chain's op: cmdgen_launch_diverse_terms (kernels_diverse.hip), then k_diverse_restrained_step_count (k_step_count
// with the restraint displacement and then the sets' displacement in the mean)
void cmdgen_launch_diverse_restrained_step(const Layout& lay, const Dims& d, const ChainBuf& c, const RestrainBuf& rb, const DiverseBuf& db,
                                           const Work& w, const float* eps, hipStream_t s);
// ... and the restrained multi-pocket chain: per op k_multi_guide (one workgroup per group: the displacement gd [Nu][3]) and then
// k_multi_restrained_step_count (one per member); RestrainBuf::rstart and op_energy are per GROUP, energy_out is [G][2]
void cmdgen_launch_multi_restrained_step(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const RestrainBuf& rb,
                                         const Work& w, const float* eps, float* gd, hipStream_t s);
// ... and the restrained multi-pocket EDIT chain: per op k_multi_edit_guide (k_multi_guide with the held rows at their given positions) and
// then k_multi_restrained_edit_step_count (k_multi_edit_step_count with the displacement in op A, on the rows whose x is not held)
void cmdgen_launch_multi_restrained_edit_step(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const InpaintBuf& ip,
                                              const RestrainBuf& rb, const Work& w, const float* eps, float* gd, hipStream_t s);
void cmdgen_launch_multi_restrain_energy(const Layout& lay, const Dims& d, const GroupTab& g, const RestrainBuf& rb, const float* xo,
                                         const float* po, float* energy_out, hipStream_t s);

// kernels_diverse.hip: the diverse chain (the conditional chain with a term that pushes the samples of a set apart).  Per op k_diverse_frame
// (the points of every sample in its caller's frame, DiverseBuf::y), k_diverse_pair (the displacement gd and op_overlap) and then
// k_diverse_step_count (k_step_count with the displacement in the mean)
void cmdgen_launch_diverse_step(const Layout& lay, const Dims& d, const ChainBuf& c, const DiverseBuf& db, const Work& w, const float* eps,
                                hipStream_t s);
// ... its first two launches alone (what the restrained diverse chain's step runs in front of its own step kernel)
void cmdgen_launch_diverse_terms(const Layout& lay, const Dims& d, const ChainBuf& c, const DiverseBuf& db, const Work& w, const float* eps,
                                 hipStream_t s);
// ... and the same two guide launches over the chain's output xo / po (A): overlap_out [B]
void cmdgen_launch_diverse_overlap(const Layout& lay, const Dims& d, const DiverseBuf& db, const float* xo, const float* po, float* overlap_out,
                                   hipStream_t s);

// kernels_multi.hip: the multi-pocket chain (groups of samples that share one latent)
void cmdgen_launch_multi_init(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const float* px, const float* poh,
                              hipStream_t s);
void cmdgen_launch_multi_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const Work& w, const float* eps,
                                    hipStream_t s);
void cmdgen_launch_multi_final(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const Work& w, const float* eps,
                               float* xo, float* po, unsigned int* cog, hipStream_t s);

// ... and the multi-pocket edit chain: the edit chain's ops on a group's shared latent (known rows and marks once per group)
void cmdgen_launch_multi_edit_start(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, float alpha, float sigma,
                                    const float* phx, const float* phoh, const float* px, const float* poh, hipStream_t s);
void cmdgen_launch_multi_edit_prep(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const InpaintBuf& ip,
                                   const float* phx, const float* phoh, const float* fix_x, const float* fix_h, const float* px,
                                   hipStream_t s);
void cmdgen_launch_multi_edit_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const GroupTab& g, const InpaintBuf& ip,
                                         const Work& w, const float* eps, hipStream_t s);

// kernels_inpaint.hip: the conditional RePaint chain and the edit chain
void cmdgen_launch_inpaint_prep(const Layout& lay, const Dims& d, const ChainBuf& c, const InpaintBuf& ip, const float* phx,
                                const float* phoh, const float* fix_x, const float* fix_h, const float* px, hipStream_t s);
void cmdgen_launch_edit_start(const Layout& lay, const Dims& d, const ChainBuf& c, const InpaintBuf& ip, float alpha, float sigma,
                              const float* phx, const float* phoh, const float* fix_x, const float* fix_h, const float* px,
                              const float* poh, hipStream_t s);
void cmdgen_launch_inpaint_step_count(const Layout& lay, const Dims& d, const ChainBuf& c, const InpaintBuf& ip, const Work& w,
                                      const float* eps, hipStream_t s);

// kernels_joint.hip: the joint model's chain
void cmdgen_launch_joint_init(const Layout& lay, const Dims& d, const JointBuf& c, const float* phx, const float* phoh,
                              const float* px, const float* poh, hipStream_t s);
void cmdgen_launch_joint_step(const Layout& lay, const Dims& d, const JointBuf& c, const float* ep, const float* eq, hipStream_t s);
void cmdgen_launch_joint_final(const Layout& lay, const Dims& d, const JointBuf& c, const float* ep, const float* eq,
                               float* xo, float* po, unsigned int* cog, hipStream_t s);

// kernels_score.hip: the scoring chain
void cmdgen_launch_score_init(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, float alpha_T, const float* phx,
                              const float* phoh, const float* px, const float* poh, float* kl_sums, hipStream_t s);
void cmdgen_launch_score_step(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const Work& w, const float* eps,
                              hipStream_t s);
void cmdgen_launch_score_final(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const Work& w, const float* eps,
                               hipStream_t s);
size_t cmdgen_score_step_lds(const Layout& lay, const Dims& d);
// ... and the multi-pocket scoring chain: groups of samples that share the clean rows and the draws (member_out: [n_levels][B][SC_COLS] or null)
void cmdgen_launch_multi_score_init(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const GroupTab& g, float alpha_T,
                                    const float* phx, const float* phoh, const float* px, const float* poh, float* kl_sums, hipStream_t s);
void cmdgen_launch_multi_score_step(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const GroupTab& g, const Work& w,
                                    const float* eps, float* member_out, hipStream_t s);
void cmdgen_launch_multi_score_final(const Layout& lay, const Dims& d, const ChainBuf& c, const ScoreBuf& sc, const GroupTab& g, const Work& w,
                                     const float* eps, float* member_out, hipStream_t s);
