// cmdgen_train_kernels.h - the interface between the training step's host side (cmdgen_train.hip) and its kernels
// (kernels_train_gemm.hip, kernels_train_dgrad.hip, kernels_train_adjoint.hip, kernels_train_repack.hip, kernels_train_loss.hip): the table structs the host fills and a kernel indexes with tab[blockIdx], the launchers with their default
// arguments, the scratch-size helpers and the launch tuning.  Both sides include this header, so each struct and each default is
// written exactly once.  Declarations only: nothing here beyond cmdgen_dev.h's types.
#pragma once
#include "cmdgen_dev.h"

// ---- per-step re-pack of the parameters into the layouts the evaluation kernels stream (fragment orders: cmdgen_wlayout.h) ----
// row_split / col_shift: rows >= row_split of the packed matrix are rows - row_split of the source, shifted col_shift columns right
// (the stacked [2H][H] projections of edge_mlp.0 / coord_mlp.0)
struct RepackFrag { int src_off, ld, out, in, row_split, col_shift; float* dst32; float* dst16; };
struct RepackMisc { int src_off, ld, rows, cols; float* dst; };      // dst[c * rows + r] = theta[src_off + r * ld + c]
// split fragment packs of transposed weight sub-blocks: dst = pack of Wt, Wt[o'][k] = theta[src_off + k * ld + o'] (o', k < 256)
struct RepackSplitT { int src_off, ld; void* dst; int transpose; };      // transpose = 0: the pack of W itself (forward: Y = X W^T)
struct RepackHalf { int src_off, ld; void* dst; float* sc; int transpose; };     // transpose: the pack of W^T (data gradients: dX = dY W)
struct RepackHalf16 { int src_off, ld, out, in, row_split, col_shift; void* dst; float* sc; };
void tr_repack(const float* theta, const void* frag_tab, int n_frag, int max_frag4, const void* misc_tab, int n_misc, int max_misc,
               hipStream_t s);
void tr_repack_split_t(const float* theta, const void* tab, int n, hipStream_t s);
void tr_repack_half(const float* theta, const void* tab, int n_plain, int n, hipStream_t s);
void tr_repack_half16(const float* theta, const void* tab, int n, int max8, hipStream_t s);

// ---- GEMMs ----
// Which kernel, grid and split-K each launcher takes is decided in cmdgen_train_plan.h; tune: the handle's TrainTune (cmdgen_handle::tune)
// split_k: 0 = choose so that the launch fills the chip (wgrad: few output tiles, K = thousands of rows); 1 = none
void cmdgen_sgemm(bool ta, bool tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                  int ldc, const float* bias, float alpha, bool accumulate, int split_k, hipStream_t s,
                  int epi = 0, float* aux = nullptr, int ldaux = 0, bool bf16 = false);
struct WgradBatch {               // up to 8 weight gradients dW (+)= dY^T X (+ bias gradients) in one launch
    const float* dy[8]; const float* x[8]; float* dw[8]; float* db[8];
    int M[8], N[8], lddy[8], ldx[8], ldw[8];
    int n;
    int xs[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // 1: X_p holds PRE-activations - SiLU is applied while the operand is staged (the forward then stores pre1 / pre6 only)
};
void cmdgen_wgrad_group(const WgradBatch& g, int K, bool bf16, hipStream_t s, const TrainTune& tune, bool split3 = false, bool force3 = false);
// pieces = 3: fp32-accurate (split engine); 1: the operands' leading bf16 piece only (= operands rounded to nearest-even
// bf16, fp32 accumulation: cmdgen_train_set_precision(1))
void cmdgen_dgrad_split(int M, const float* A0, const void* W0, const float* A1, const void* W1, float* Y, bool accumulate, float div,
                        const float* pre, hipStream_t s, const TrainTune& tune, int pieces = 3, const void* W0b = nullptr, float* Yb = nullptr,
                        bool accumulate_b = false, float div_b = 1.0f, int force_mt = 0, const float* Yin = nullptr, const float* rowdiv_b = nullptr);
void cmdgen_dgrad_tail(int E, const float* dY, const void* Wt, const float* pre1, const int* row, const int* col, const float* d0,
                       const float* Wcol, int ldw, const float4* X, float nc, const float4* dcd, int n_moving, float* dP, float* dQ,
                       float* dWcol, float* dX, float* scratch, int pieces, hipStream_t s, unsigned long long* dbg, bool defer_reduce = false,
                       const float* Wd = nullptr, float* dd0 = nullptr);      // dbg: Work::dbg, for the stamped diagnostic build (tools/tail_stamps.py)

// ---- adjoints of the edge models' element-wise parts, with their parameter reductions ----
size_t tr_partial_scratch_floats(size_t E, size_t H);
size_t tr_edge_tail_scratch_floats(size_t E, size_t H);
void tr_reduce_pair(int E, int H, const float* scratch_a, float* out_w, float* out_b, const float* scratch_t, float* dWcol, int ldw, hipStream_t s);
void tr_gate_bwd(int E, int H, const int* row, const float* pre2, const float* wa, const float* z, int attention, const float* dagg,
                 float* dpre2, float* scratch, float* d_wa, float* d_ba, float* zero, size_t zero_floats, hipStream_t s,
                 bool defer_reduce = false);
// the inputs of coord_out_edge (cmdgen_train_parts.h), for the form of k_head_bwd that computes dphi (and writes dcd) itself: one launch less per block
struct CoordOutArgs { const int* row; const int* col; const float4* X; const float* phi; int use_tanh; float range, norm_constant;
                      const float* dacc; float dacc_div; const float* adiv; float4* dcd_out; };
void tr_head_bwd(int E, int H, const float* dphi, const float* w5, const float* pre7, float* dpre7, float* scratch, float* d_w5,
                 float* zero, size_t zero_floats, hipStream_t s, bool defer_reduce = false, const CoordOutArgs* co = nullptr);
void tr_edge_tail_bwd(int E, int H, const int* row, const int* col, const float* g, const float* d0, const float* Wcol, int ldw,
                      const float4* X, float nc, const float4* dcd, int n_moving, float* dP, float* dQ, float* dWcol, float* dX,
                      float* scratch, hipStream_t s, const float* Wd = nullptr, float* dd0 = nullptr);
void tr_d0_adjoint(int E, const int* row, const int* col, const float4* X0, const float* dd0, float* dX, hipStream_t s);

// ---- small element-wise and reduction launches ----
void tr_silu_bwd(float* g, const float* pre, size_t n, hipStream_t s);
void tr_scale(float* x, float d, size_t n, hipStream_t s);
void tr_scale_rows(float* x, const float* div, int H, size_t n, hipStream_t s);
void tr_colsum(int E, int ncols, const float* X, int ldx, const float* sv, float* out, int ldo, hipStream_t s);
void tr_center_per_sample(const Layout& lay, float* v, hipStream_t s);
void tr_eps_bwd(int n_rows, int F, int row0, const float* deps, float* dvel, float* ddec, hipStream_t s);
void tr_bwd_init(int Nl, int N, int P, int dyn, const float* deps, float* dX, float* ddec, float* dhfin, hipStream_t s);
void tr_zero_if_flag(float* v, size_t n, const int* flag, hipStream_t s);
void tr_input_x(int Nl, int N, int ldp, int ldq, const float* dX, const float* dvel0, const int* nan_flag, float* dxp, float* dxq, hipStream_t s);
void tr_dt(const Layout& lay, const float* dhdyn, int dyn, float* dt, hipStream_t s);

// ---- optimizer, gradient norm and the half engine's range guard ----
void tr_adamw(size_t n, float* theta, const float* grad, float* m, float* v, float* vmax, float lr, float b1, float b2,
              float eps, float wd, float bias1, float bias2_sqrt, float clip, hipStream_t s, const float* sqnorm = nullptr,
              float max_norm = 0.f, int skip_nonfinite = 0);
void tr_sqsum(size_t n, const float* x, float* out, hipStream_t s);
void tr_low_snap(const unsigned long long* counters, unsigned* snap, hipStream_t s);
void tr_range_event(const int* nan_flag, const unsigned long long* counters, const unsigned* snap, float* out, hipStream_t s);
void tr_norm_guard(float* sq, const float* shared, const int* nan_flag, const unsigned long long* counters, const unsigned* snap, hipStream_t s);

// ---- noising and the loss ----
void tr_noise(const Layout& lay, const Dims& d, const float* px, const float* poh, const float* qx, const float* qoh, const float* tab,
              const float* eps, float* z_t, float* xh_pocket, float* klsum, hipStream_t s);
void tr_noise_joint(const Layout& lay, const Dims& d, const float* px, const float* poh, const float* qx, const float* qoh, const float* tab,
                    const float* raw_l, const float* raw_q, float* z_l, float* z_q, float* e_l, float* e_q, float* klsum, hipStream_t s);
void tr_loss(const Layout& lay, const Dims& d, int l2, float T, const float* net, const float* eps, const float* z_t, const float* poh,
             const float* tab, const float* klsum, float* terms, float* d_eps, float* means, hipStream_t s);
void tr_loss_joint(const Layout& lay, const Dims& d, int l2, float T, const float* net_l, const float* net_q, const float* e_l, const float* e_q,
                   const float* z_l, const float* z_q, const float* poh, const float* qoh, const float* tab, const float* klsum, float* terms,
                   float* d_l, float* d_q, float* means, hipStream_t s);
