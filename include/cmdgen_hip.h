/*
 * cmdgen_hip.h - C ABI of libcmdgen_hip.so: the MI355X (gfx950) implementation of
 * DiffPhar's pocket-conditioned denoising path.
 *
 * The reference (zyrlia1018/CMD-GEN, DiffPhar/) is pure Python and has no FFI of its
 * own; the entry points below are what a binding for this path replaces, cited as
 * file:line relative to /root/reference/DiffPhar.  INTEGRATION.md shows the ctypes
 * stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  "dev" pointers are device memory
 *     owned by the CALLER (e.g. torch tensors' data_ptr()); "host" pointers are host
 *     memory.  The handle owns packed weights, the schedule table, workspaces and
 *     hipGraph executables, nothing else.
 *   - Every launch goes to the caller-supplied stream; no hidden device synchronise
 *     except where a function is documented to return host-visible results.
 *   - Return 0 on success, a negative CMDGEN_E* code otherwise; cmdgen_last_error()
 *     gives the message.  Nothing throws across the ABI.
 *   - A handle is bound to one device and is not thread-safe (one handle per GPU /
 *     host thread), like the reference's module objects.
 *   - Flat, un-padded node lists (PyG style): all samples' nodes concatenated along
 *     dim 0, sample membership given by per-sample counts; masks must be ascending
 *     and contiguous, as every mask the reference builds is (utils.py:137-145,
 *     dataset.py:59-60, lightning_modules.py:445-448).
 *   - All floating point is fp32 (constants.py:8).
 */
#ifndef CMDGEN_HIP_H
#define CMDGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMDGEN_OK            0
#define CMDGEN_EINVAL       -1   /* bad argument / unsupported configuration */
#define CMDGEN_ESTATE       -2   /* call order (weights not finalised, no layout, ...) */
#define CMDGEN_EHIP         -3   /* a HIP runtime call failed */
#define CMDGEN_ENOMEM       -4

typedef struct cmdgen_handle cmdgen_handle;
typedef void* cmdgen_stream;     /* hipStream_t */

/* Hyper-parameters that fix every shape on the path
 * (EGNNDynamics.__init__ dynamics.py:10-73, EGNN.__init__ egnn_new.py:160-191,
 *  EnVariationalDiffusion.__init__ en_diffusion.py:18-62; values of
 *  configs/crossdocked_ca_cond.yml:22-41 in comments). */
typedef struct cmdgen_config {
    int32_t phar_nf;               /* 8  */
    int32_t residue_nf;            /* 20 (CA) or 11 (full-atom) */
    int32_t joint_nf;              /* 32 */
    int32_t hidden_nf;             /* 256; one of 64, 128, 256, 512 (512: sampling only, fp32-image tiles; the plane kernels are 256 only) */
    int32_t n_layers;              /* 5  */
    int32_t inv_sublayers;         /* 1; GCLs per EquivariantBlock (egnn_new.py:127-131): >= 1 for sampling (dead-work skipping is off above 1),
                                      the training step supports 1 only */
    int32_t attention;             /* 1  */
    int32_t tanh;                  /* 1  */
    int32_t condition_time;        /* 1  */
    int32_t timesteps;             /* T of the gamma table (500) */
    int32_t no_com_projection;     /* 0; 1 = SimpleConditionalDDPM (conditional_model.py:481-525): pocket centred once,
                                      no centre-of-mass projection of the samples */
    int32_t update_pocket_coords;  /* 0; 1 = mode 'joint' (lightning_modules.py:125, dynamics.py:105-107, :133-136):
                                      pocket nodes move too and the velocity's centre of mass is removed;
                                      required by cmdgen_joint_chain */
    float   edge_cutoff;           /* 6.0; < 0 means no cutoff (complete graph per sample) */
    float   norm_constant;         /* 1  */
    float   normalization_factor;  /* 100 (aggregation_method 'sum': segment sums are divided by it, egnn_new.py:285-286) */
    float   coords_range;          /* 15 (egnn_new.py:161; quirk: never divided by n_layers) */
    float   norm_x;                /* norm_values[0] = 1 */
    float   norm_h;                /* norm_values[1] = 4 */
    float   bias_h;                /* norm_biases[1] = 0 */
    int32_t aggregation_mean;      /* 0 = aggregation_method 'sum'; 1 = 'mean' (egnn_new.py:288-292: every segment sum is divided by its
                                      receiver's edge count instead of normalization_factor); sampling only */
    int32_t sin_embedding;         /* 0; 1 = SinusoidsEmbeddingNew on both distance features of an edge (egnn_new.py:174-176, :249-260: the
                                      first layer of the edge / coordinate MLPs has 2H + 24 inputs); sampling only, on the fp32 matrix
                                      instruction (the plane kernels of the split engine carry the two scalar features only) */
} cmdgen_config;

/* Work counters accumulated on the device since the last reset (for the
 * algorithmic-FLOP roofline). */
typedef struct cmdgen_counters {
    uint64_t evaluations;          /* network evaluations (EGNNDynamics.forward calls) */
    uint64_t edges;                /* sum over evaluations of directed edges incl. self loops */
    uint64_t edges_phar;           /* ... of those the coordinate update runs on: receiver is a pharmacophore node and
                                      the edge is not a self loop (a self loop's coord_diff is exactly 0) */
    uint64_t nodes;                /* sum over evaluations of nodes */
    uint64_t nan_resets;           /* evaluations whose velocity was reset (dynamics.py:129-131) */
    uint64_t edges_skipped;        /* edges of k_edge_msg tiles that were skipped as dead work (last block of a conditional evaluation: no receiver
                                      of the tile is still read), summed over launches: the executed edge work is edges * n_layers - this */
    uint64_t node_rows_skipped;    /* rows of k_node tiles skipped for the same reason, summed over launches */
    uint64_t half_low_range;       /* valid rows of the half matrix engine's SiLU-output A operands (edge / coordinate MLP first layers, the
                                      node MLP's hidden layer) whose max |a| lies below 2^-5 (over all of K, or over one quarter of K in the
                                      128-row edge and the plane node tiles): there the products lose fp32 accuracy silently (cmdgen_split.h,
                                      HALF_LOW_TAU); replayed graphs included.  A non-zero delta over a call: repeat it on the three-piece
                                      bf16 split ("half_engine" = 0) */
} cmdgen_counters;

/* Per-kernel timing of one profiled evaluation (hipEvent pairs on the launch stream). */
typedef struct cmdgen_kernel_times {
    float edge_build_ms, embed_ms, edge_msg_ms, node_ms, edge_coord_ms, readout_ms, ddpm_ms;
    int32_t edge_msg_launches, node_launches, edge_coord_launches;
} cmdgen_kernel_times;

/* ---- lifetime --------------------------------------------------------------------- */
/* Replaces constructing EGNNDynamics + ConditionalDDPM (lightning_modules.py:110-139). */
int  cmdgen_create(const cmdgen_config* cfg, int device, cmdgen_handle** out);
void cmdgen_destroy(cmdgen_handle* h);
const char* cmdgen_last_error(const cmdgen_handle* h);   /* h may be NULL: last create error */
const char* cmdgen_version(void);

/* ---- parameters ------------------------------------------------------------------- */
/* Replaces nn.Module.load_state_dict for the 'ddpm.' sub-tree of a Lightning checkpoint
 * (generate_phars.py:32).  `name` is the reference key below 'ddpm.', e.g.
 * "dynamics.egnn.e_block_0.gcl_0.edge_mlp.0.weight" or "gamma.gamma"; `host` holds `n`
 * fp32 values in nn.Linear layout [out, in] row-major. */
int cmdgen_load_weights(cmdgen_handle* h, const char* name, const float* host, size_t n);
/* Checks that every tensor arrived, packs them into MFMA fragment order on the device. */
int cmdgen_finalize_weights(cmdgen_handle* h);

/* ---- batch layout ----------------------------------------------------------------- */
/* Per-sample node counts of the flat batch (host arrays of length `batch`):
 * num_phar = num_nodes_phar, num_pocket = pocket['size'] (conditional_model.py:388-408).
 * Sizes workspaces; cheap when the layout is unchanged. */
int cmdgen_set_layout(cmdgen_handle* h, int64_t batch,
                      const int64_t* num_phar_host, const int64_t* num_pocket_host);
/* Ordering contract: the call rewrites index arrays that kernels of the PREVIOUS layout read.  Before touching
 * them it waits for the stream most recently passed to this handle (and its internal stream); work the caller
 * queued for this handle on any OTHER stream must be complete before calling.  Limits: a sample's nodes are kept
 * in LDS by the neighbour search (24 B per node; at most ~6500 nodes per sample), the dense edge bound
 * sum(n_b^2) must fit int32. */
/* The same, ordered on `stream` instead of waited for: when the new layout fits the workspaces already allocated (every
 * training step has its own ragged layout of about the same size) and `stream` is the stream this handle was last given,
 * the index arrays are written to the second of two device blocks from pinned staging with a stream-ordered copy, so
 * kernels of the previous layout still running on `stream` are not disturbed and the host does not wait.  Otherwise it
 * behaves as cmdgen_set_layout (and also waits for `stream`). */
int cmdgen_set_layout_on_stream(cmdgen_handle* h, int64_t batch, const int64_t* num_phar_host,
                                const int64_t* num_pocket_host, cmdgen_stream stream);

/* ---- one network evaluation ------------------------------------------------------- */
/* EGNNDynamics.forward (dynamics.py:75-139); conditional mode, or joint mode when
 * config.update_pocket_coords = 1 (then eps_pocket is required: its x columns are the pocket velocity).
 *   xh_phar   dev [Nl, 3+phar_nf]      xh_pocket dev [Np, 3+residue_nf]
 *   t         dev [batch]              (the reference's [B,1]; a single-sample batch uses t[0])
 *   eps_phar  dev [Nl, 3+phar_nf]  out
 *   eps_pocket dev [Np, 3+residue_nf] out, may be NULL (every conditional caller discards it:
 *              conditional_model.py:115, :246, :355) */
int cmdgen_dynamics_forward(cmdgen_handle* h, const float* xh_phar, const float* xh_pocket,
                            const float* t, float* eps_phar, float* eps_pocket,
                            cmdgen_stream stream);

/* Radius graph of the last evaluation, EGNNDynamics.get_edges (dynamics.py:141-147):
 * copies up to `cap` edges as (row, col) int32 pairs in the reference's flat node
 * numbering (phar nodes first) to HOST arrays; returns the edge count in *n_edges.
 * Synchronises the stream.  Debug / parity aid. */
int cmdgen_get_edges(cmdgen_handle* h, int32_t* row_host, int32_t* col_host, int64_t cap,
                     int64_t* n_edges, cmdgen_stream stream);

/* EGNNDynamics.get_edges(batch_mask, x) (dynamics.py:141-147) for ARBITRARY coordinates, independent of the
 * handle's batch layout: x dev [sum counts, 3] holds `batch` samples back to back (ascending mask), counts_host
 * their sizes.  Writes the edges (same sample, ||x_i - x_j|| <= edge_cutoff, self loops kept) sorted by (row, col)
 * to the DEVICE arrays row_dev / col_dev (int32, capacity `cap` >= sum counts^2, else CMDGEN_EINVAL) and the
 * count to *n_edges.  Synchronises the stream. */
int cmdgen_radius_graph(cmdgen_handle* h, const float* x, const int64_t* counts_host, int64_t batch,
                        int32_t* row_dev, int32_t* col_dev, int64_t cap, int64_t* n_edges, cmdgen_stream stream);

/* Parity aid: run one evaluation only up to a point, so that intermediates the fused kernels never keep can be
 * read with cmdgen_debug_read: all of blocks 0..block-1, then of block `block` stage 1 = after the edge-message
 * kernel ("agg" holds the un-normalised segment sums of e_ij, egnn_new.py:50-52), 2 = after the node kernel ("h"
 * is the block's output, "agg" is zero again), 3 = after the coordinate kernel ("acc" row `block` holds the sums
 * of trans, egnn_new.py:91-98).  Leaves the workspace unusable for a chain until the next full evaluation. */
int cmdgen_debug_eval_prefix(cmdgen_handle* h, const float* xh_phar, const float* xh_pocket, const float* t,
                             int32_t block, int32_t stage, cmdgen_stream stream);

/* Copy an internal activation of the last evaluation to host (parity aid): what = "h" | "agg" | "P" | "Q" [N, hidden],
 * "x0" [Nm, 4], "xl" / "acc" [n_layers, Nm, 4].  After a CONDITIONAL evaluation whose pocket output was not requested
 * (eps_pocket == NULL, every chain) the POCKET rows of h / P / Q are undefined unless option "dead_skip" is 0: blocks skip
 * tiles whose result nobody reads, so those rows hold a mix of earlier blocks.  Phar rows, agg (zero) and the positions are
 * always complete; cmdgen_debug_eval_prefix never skips.
 * "chain_z" [Nl, 3 + phar_nf]: the z buffer of the last conditional chain (sample, inpaint / edit, multi-pocket, multi-pocket edit) as
 * its decode left it - for the multi-pocket chains EVERY member's copy of the group's latent, which are equal bit for bit. */
int cmdgen_debug_read(cmdgen_handle* h, const char* what, float* host, size_t n, cmdgen_stream stream);

/* Fills out_dev[n_nodes * width] with the standard normals the sampler would draw for draw index
 * `draw`, global pocket id `pocket_id` (Philox4x32-10 + Box-Muller; the production noise source of
 * cmdgen_sample_chain when `noise` is NULL).  Test aid for the statistical checks. */
int cmdgen_debug_noise(cmdgen_handle* h, uint64_t seed, int64_t pocket_id, int32_t draw, int32_t n_nodes,
                       int32_t width, float* out_dev, cmdgen_stream stream);

/* ---- the denoising loop ----------------------------------------------------------- */
/* ConditionalDDPM.sample_given_pocket (conditional_model.py:388-465) with return_frames=1:
 * init noise around the pocket COM, `timesteps` posterior steps (sample_p_zs_given_zt
 * :342-374), final p(x,h|z0) decode (:108-131), CoG drift fix (:451-457).
 *   pocket_x      dev [Np, 3]           un-normalised coordinates
 *   pocket_onehot dev [Np, residue_nf]  one-hot (un-normalised; scaled by 1/norm_h inside)
 *   timesteps     K <= T, strided schedule t=(s+1)/K as the reference
 *   noise         dev [K+2, Nl, 3+phar_nf] Gaussian draws in the reference's draw order, or
 *                 NULL to draw on the device (Philox4x32-10 keyed by seed, global pocket id,
 *                 draw index, node) - the reference draws with torch.randn on the compute
 *                 device (en_diffusion.py:946-949), which no other device can reproduce.
 *   pocket_ids_host  host [batch] global pocket indices for the Philox key (NULL: 0..batch-1);
 *                 makes results independent of how pockets are sharded over GPUs.
 *   xh_phar_out   dev [Nl, 3+phar_nf]    x in Angstrom, h one-hot (as floats)
 *   xh_pocket_out dev [Np, 3+residue_nf] translated pocket, h = one_hot
 *   z_steps_out   dev [K, Nl, 3+phar_nf] z after each posterior step, or NULL
 *   pocket_steps_out dev [K, Np, 3] translated pocket coordinates after each step (normalised space), or NULL
 *                 (both feed return_frames > 1, conditional_model.py:439-442)
 *   use_graph     1: replay the step as a hipGraph, 0: eager launches
 * Asynchronous on `stream`; call cmdgen_chain_status afterwards for the deferred checks. */
int cmdgen_sample_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                        int32_t timesteps, const float* noise, uint64_t seed,
                        const int64_t* pocket_ids_host,
                        float* xh_phar_out, float* xh_pocket_out, float* z_steps_out,
                        float* pocket_steps_out, int32_t use_graph, cmdgen_stream stream);

/* One pharmacophore for SEVERAL pockets (ConditionalDDPM.sample_given_pockets): cmdgen_sample_chain's chain with one latent z per
 * GROUP of pocket contexts - two targets of a dual-target design, or several conformations of one receptor.  At every op the
 * eps-predictions of the group's contexts are combined with weights, the score of the weighted geometric mixture of the per-pocket
 * distributions.  The layout (cmdgen_set_layout) holds the B = sum_g M_g MEMBER samples: the members of group g are the consecutive
 * samples first[g] .. first[g] + M_g - 1, all with the same n_phar; their pockets differ freely in size and composition and are
 * given in ONE common frame (superposing them is the caller's business).  Nu = sum_g n_phar[g] counts one copy of the rows per group.
 * In the normalised space, with P_m the pocket of member m, w_m its weight and sums over m ascending:
 *   Init    c = sum_m w_m com(P_m);  z = [c, 0] + xi_0;  shift = com(z.x);  z.x -= shift and every P_m.x -= shift;  the mean-zero check.
 *   Op t->s eps_m = the phar output of the ordinary evaluation of (z, P_m, t), its x columns zero when the (batch-wide) NaN guard is set;
 *           eps_bar = sum_m w_m eps_m;  mu = z / alpha_ts - c_eps eps_bar;  z' = mu + sigma xi;  shift = com(z'.x);
 *           z'.x -= shift and every P_m.x -= shift.  The scalars are the step table's (cmdgen_set_step_table), as cmdgen_sample_chain.
 *   Final   eps_bar at t = 0;  x = (z - sigma_0 eps_bar) / alpha_0 + sigma_x xi;  the COM is removed from x and every P_m;  types =
 *           argmax of z_0;  unnormalise;  the CoG-drift re-centring is batch-wide as in cmdgen_sample_chain.
 * The shared latent stays COM-free and every pocket carries its own translated copy of the frame.  With every M_g = 1 this is
 * cmdgen_sample_chain, bit for bit.
 *   pocket_x, pocket_onehot  as cmdgen_sample_chain, the rows of the B member samples in layout order
 *   n_groups, group_size_host int64 [n_groups]: M_g in 1 .. CMDGEN_MAX_GROUP, summing to the layout's batch
 *   weight_host   float [batch], one per member: >= 0, finite, each group's summing to 1 within 1e-5 (the caller normalises)
 *   noise  dev [K+2][Nu][3+phar_nf] or NULL: ONE draw per group and op, in cmdgen_sample_chain's order (draw 0: xi_0, 1 + i: op i,
 *          1 + K: the decode); all members of a group use the same numbers.
 *   Device draws (noise == NULL): Philox keyed by (seed, global GROUP id, draw, node of the group) with those draw counters -
 *          cmdgen_debug_noise(seed, group id, draw, n_phar, ...) returns the same numbers.
 *   group_ids_host  host [n_groups] global group ids for the Philox key (NULL: 0 .. n_groups-1)
 *   xh_phar_out dev [Nu][3+phar_nf];  xh_pocket_out dev [Np][3+residue_nf]: every member's translated pocket;
 *   z_steps_out dev [K][Nu][3+phar_nf] or NULL;  pocket_steps_out dev [K][Np][3] or NULL: as cmdgen_sample_chain
 * One op is one launch (k_multi_step_count: one workgroup per member, each with its own copy of z - no float atomics, no
 * synchronisation between workgroups) plus the evaluation; with use_graph the step is captured and replayed like the other chains, and
 * a changed grouping or weight prepares the chain's slot again.
 * Refused: n_phar unequal inside a group, sizes that do not sum to the batch or lie outside 1 .. CMDGEN_MAX_GROUP, a negative or
 * non-finite weight, a group whose weights do not sum to 1, the joint model and no_com_projection handles (SimpleConditionalDDPM).
 * Asynchronous on `stream`; cmdgen_chain_status reports this run's checks, drift and NaN resets. */
#define CMDGEN_MAX_GROUP 8
int cmdgen_multi_pocket_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                              int64_t n_groups, const int64_t* group_size_host, const float* weight_host,
                              int32_t timesteps, const float* noise, uint64_t seed, const int64_t* group_ids_host,
                              float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                              int32_t use_graph, cmdgen_stream stream);

/* The JOINT model's loops (config.update_pocket_coords = 1), return_frames=1:
 *   phar_fixed == NULL && pocket_fixed == NULL: EnVariationalDiffusion.sample (en_diffusion.py:576-647) -
 *       phar AND pocket nodes start from noise; phar_x/phar_onehot/pocket_x/pocket_onehot are ignored (may be NULL).
 *   otherwise: EnVariationalDiffusion.inpaint (en_diffusion.py:672-831), RePaint with the schedule of
 *       get_repaint_schedule(resamplings, jump_length, timesteps) (:649-670).  generate_phars' inpainting
 *       branch (lightning_modules.py:466-486) passes phar_x = 0, phar_onehot = 0, phar_fixed = 0, pocket_fixed = 1.
 *   phar_x dev [Nl,3], phar_onehot dev [Nl,phar_nf], pocket_x dev [Np,3], pocket_onehot dev [Np,residue_nf]:
 *       used RAW - the reference's inpaint never calls normalize (quirk kept);
 *   phar_fixed dev [Nl], pocket_fixed dev [Np]: 1.0 = known node, 0.0 = node to generate;
 *   noise  dev [n_draws][Nl*(3+phar_nf) + Np*(3+residue_nf)] or NULL (Philox on the device).  One row per
 *       sample_combined_position_feature_noise call (:555-574) in the reference's call order: the phar block
 *       [Nl,3+phar_nf] then the pocket block [Np,3+residue_nf]; x columns hold the raw draw (the centre-of-mass
 *       projection is applied inside).  Draws: 1 (z_T) + per denoising step [1 if inpainting: known part] + 1
 *       + [1 if the step is followed by a jump back] + 1 (final decode);
 *   n_draws  rows available in `noise` (checked against the schedule; ignored when noise == NULL);
 *   xh_phar_out dev [Nl,3+phar_nf], xh_pocket_out dev [Np,3+residue_nf]: x, one-hot h (floats);
 *   z_steps_out dev [n_steps][Nl*(3+phar_nf) + Np*(3+residue_nf)] or NULL: z after every denoising step
 *       (after the known/unknown merge, before any jump back); n_steps = sum of the schedule.
 * Asynchronous on `stream`; cmdgen_chain_status reports the deferred mean-zero checks / CoG drift. */
int cmdgen_joint_chain(cmdgen_handle* h, const float* phar_x, const float* phar_onehot,
                       const float* pocket_x, const float* pocket_onehot,
                       const float* phar_fixed, const float* pocket_fixed,
                       int32_t timesteps, int32_t resamplings, int32_t jump_length,
                       const float* noise, int64_t n_draws, uint64_t seed, const int64_t* pocket_ids_host,
                       float* xh_phar_out, float* xh_pocket_out, float* z_steps_out,
                       int32_t use_graph, cmdgen_stream stream);

/* Number of denoising steps (= network evaluations - 1) and of combined noise draws cmdgen_joint_chain will use. */
int cmdgen_joint_plan(cmdgen_handle* h, int32_t timesteps, int32_t resamplings, int32_t jump_length,
                      int32_t inpaint, int64_t* n_steps, int64_t* n_draws);

/* RePaint for the CONDITIONAL model (ConditionalDDPM.inpaint): sample_given_pocket's chain with the rows of phar_fixed
 * held at a noised copy of the given rows.  The schedule is get_repaint_schedule(resamplings, jump_length, timesteps)
 * (en_diffusion.py:649-670), walked as en_diffusion.py:723-813 do; one op going from t to s, in the normalised space:
 *   A  (z_u, P_u) = sample_p_zs_given_zt(s, t, z, P)                                 (conditional_model.py:342-374)
 *   B  z_k = alpha_s K + sigma_s eps_B over all phar rows; z_k.x += com(P_u) - com(P0) per sample;
 *      z = phar_fixed ? z_k : z_u; (z.x, P.x) = remove_mean_batch(z.x, P_u.x)        (skipped for a sample with no fixed row)
 *   C  after the last op before a jump back: (z, P) = sample_p_zt_given_zs(z, P, gamma(s + jump_length), gamma(s))
 * K = the normalised phar input rows, P0 = the normalised input pocket, P = its translated copy (the phar COM stays at 0).
 * z_T and the final decode (with the CoG-drift projection) are sample_given_pocket's.  With resamplings = jump_length = 1
 * a sample without fixed rows follows cmdgen_sample_chain's trajectory bit for bit (same seed, device draws).
 *   pocket_x, pocket_onehot      as cmdgen_sample_chain (raw; normalised on the device)
 *   phar_x dev [Nl,3], phar_onehot dev [Nl,phar_nf]: raw input phar rows (only fixed rows are read)
 *   phar_fixed dev [Nl]: nonzero = fixed row
 *   noise  dev [n_draws][Nl][3+phar_nf] or NULL, in call order: draw 0 (z_T); per op draw A, draw B, and draw C if the op
 *          jumps back; the decode draw.  n_draws = 2 + 2 n_steps + n_jumps (cmdgen_inpaint_plan); fewer rows are refused.
 *   Device draws (noise == NULL): Philox keyed by (seed, global pocket id) as cmdgen_sample_chain, with the draw counter
 *          z_T: 0, A of op i: 1 + i, decode: 1 + n_steps, B of op i: 2 + n_steps + i, C of op i: 2 + 2 n_steps + i.
 *   outputs as cmdgen_sample_chain; z_steps_out [n_steps][Nl][3+phar_nf] and pocket_steps_out [n_steps][Np][3] hold z and
 *          P after step B of every op (before a jump back).
 * The joint model (use cmdgen_joint_chain) and no_com_projection handles (SimpleConditionalDDPM) are refused.
 * Asynchronous on `stream`; cmdgen_chain_status reports this run's checks, drift and NaN resets. */
int cmdgen_inpaint_plan(cmdgen_handle* h, int32_t timesteps, int32_t resamplings, int32_t jump_length,
                        int64_t* n_steps, int64_t* n_draws);
int cmdgen_inpaint_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                         const float* phar_x, const float* phar_onehot, const float* phar_fixed,
                         int32_t timesteps, int32_t resamplings, int32_t jump_length,
                         const float* noise, int64_t n_draws, uint64_t seed, const int64_t* pocket_ids_host,
                         float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                         int32_t use_graph, cmdgen_stream stream);

/* The edit chain (ConditionalDDPM.edit): cmdgen_inpaint_chain with a mask per column group and a start level, to MODIFY a given
 * pharmacophore - hold the types and re-place the points, hold the positions and re-type them, or perturb it by a chosen amount.
 * Notation as above (K the normalised given rows, P0 the normalised input pocket, P its translated copy), timesteps = Kt.
 *   Ops.  A and C as cmdgen_inpaint_chain.  B forms z_k = alpha_s K + sigma_s eps_B over all rows and z_k.x += com(P_u) - com(P0),
 *      then merges per column group:  z.x = fix_x ? z_k.x : z_u.x,  z.h = fix_h ? z_k.h : z_u.h,  then
 *      (z.x, P.x) = remove_mean_batch(z.x, P_u.x).  A sample with no mark in either mask skips B.
 *   Start.  start == timesteps: z_T around the pocket centre, as cmdgen_sample_chain.  start < timesteps: the forward process of the
 *      given rows as ConditionalDDPM.forward forms it (conditional_model.py:235-243): K.x and P0.x centred on the phar centre of mass
 *      of the sample's given rows, z = alpha(start / Kt) xh0 + sigma(start / Kt) eps_0, remove_mean_batch(z.x, P.x) and the mean-zero
 *      check; then ALL rows of phar_x and phar_onehot are read, not only marked ones.  The ops walk s = start-1 .. 0 on the Kt grid
 *      with get_repaint_schedule(resamplings, jump_length, start); the posterior rows are those of the Kt step table at the same s.
 *   fix_x, fix_h dev [Nl]: nonzero = the row's x columns / its phar_nf feature columns are held
 *   start  in 1 .. timesteps (others are refused)
 *   noise  dev [n_draws][Nl][3+phar_nf] or NULL, in call order: draw 0 (z_T or eps_0); per op draw A, draw B, and draw C if the op
 *          jumps back; the decode draw.  n_draws = 2 + 2 n_steps + n_jumps for the schedule actually walked (cmdgen_edit_plan).
 *   Device draws: the Philox counters of cmdgen_inpaint_chain with that n_steps -
 *          draw 0: 0, A of op i: 1 + i, decode: 1 + n_steps, B of op i: 2 + n_steps + i, C of op i: 2 + 2 n_steps + i.
 *   everything else as cmdgen_inpaint_chain, which is this entry with fix_x = fix_h = phar_fixed and start = timesteps, bit for bit
 *          (the two share one slot of the handle: a changed start or plan prepares it again, the caller's pointers stay the graph key).
 * One op is one launch (k_inpaint_step_count) plus the evaluation, as for inpainting.  Refusals as cmdgen_inpaint_chain. */
int cmdgen_edit_plan(cmdgen_handle* h, int32_t timesteps, int32_t start, int32_t resamplings, int32_t jump_length,
                     int64_t* n_steps, int64_t* n_draws);
int cmdgen_edit_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                      const float* phar_x, const float* phar_onehot, const float* fix_x, const float* fix_h,
                      int32_t timesteps, int32_t start, int32_t resamplings, int32_t jump_length,
                      const float* noise, int64_t n_draws, uint64_t seed, const int64_t* pocket_ids_host,
                      float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                      int32_t use_graph, cmdgen_stream stream);

/* Hold or edit given points while sampling ONE pharmacophore for several pockets (ConditionalDDPM.edit_given_pockets): the ops of
 * cmdgen_edit_chain on the shared latent of cmdgen_multi_pocket_chain.  Layout, groups, weights, group_ids_host and the outputs are
 * exactly cmdgen_multi_pocket_chain's (B member samples, Nu = one copy of the phar rows per group); start, resamplings, jump_length and
 * the draw order are exactly cmdgen_edit_chain's, and cmdgen_edit_plan gives n_steps and n_draws (the plan does not depend on the
 * grouping).  In the normalised space, with P_m the translated pocket of member m, P0_m its normalised input, K the normalised given
 * rows of the group, w_m the weights, sums over m ascending and "first" the group's first member:
 *   Init    start == timesteps: cmdgen_multi_pocket_chain's, on draw 0.  start < timesteps: cK = com(K) over the group's rows;
 *           xh0 = [K.x - cK, K.h] and every P_m.x = P0_m.x - cK;  z = alpha(start / Kt) xh0 + sigma(start / Kt) eps_0;  shift = com(z.x);
 *           z.x -= shift and every P_m.x -= shift;  the mean-zero check (cmdgen_edit_chain's expressions).  Then ALL rows of phar_x and
 *           phar_onehot are read.
 *   Offset  off = com(P_first) - com(P0_first), the frame offset of the GROUP, taken once after the init from the first member's rows
 *           as cmdgen_inpaint_chain takes it for its one pocket.  Afterwards it only changes by the means subtracted from z.  All
 *           pockets of a group sit in one frame and move by the same shifts, so this is com(P_m) - com(P0_m) of every member up to
 *           rounding - and z depends on eps_bar, the draws, K and off alone, so the members' copies of z stay bit-identical.
 *   A       cmdgen_multi_pocket_chain's op on eps_bar = sum_m w_m eps_m (x columns zero under the batch-wide NaN guard), then the COM
 *           projection of z and of every P_m;  off -= shift.
 *   B       z_k = alpha_s K + sigma_s eps_B over the group's rows; z_k.x += off;  z.x = fix_x ? z_k.x : z_u.x,  z.h = fix_h ? z_k.h : z_u.h;
 *           shift = com(z.x);  z.x -= shift, every P_m.x -= shift, off -= shift.  A group with no mark in either mask skips B.
 *   C       before a jump back: z = alpha_t'|s z + sigma_t'|s xi_C, then the same projection; off follows it.
 *   Final   cmdgen_multi_pocket_chain's decode and CoG-drift re-centring.
 *   phar_x dev [Nu,3], phar_onehot dev [Nu,phar_nf], fix_x, fix_h dev [Nu]: one row per unique phar row, raw, in the pockets' common
 *          frame; normalised on the device.  From the prior only marked column groups are read.
 *   noise  dev [n_draws][Nu][3+phar_nf] or NULL: ONE draw per group, op and role, in cmdgen_edit_chain's call order; fewer rows than
 *          the plan needs are refused.
 *   Device draws: Philox keyed by (seed, global GROUP id, counter, node of the group) with cmdgen_edit_chain's counters -
 *          draw 0: 0, A of op i: 1 + i, decode: 1 + n_steps, B of op i: 2 + n_steps + i, C of op i: 2 + 2 n_steps + i.
 *   z_steps_out dev [n_steps][Nu][3+phar_nf] or NULL (written by the group's first member), pocket_steps_out dev [n_steps][Np][3] or
 *          NULL (every member's pocket): the state after B of every op, before a jump back.
 * With every M_g = 1 this is cmdgen_edit_chain, and with no mark, start = timesteps and resamplings = jump_length = 1 it is
 * cmdgen_multi_pocket_chain, both bit for bit (same seed, device draws or injected noise).
 * One op is one launch (k_multi_edit_step_count: one workgroup per member, no float atomics, no synchronisation between workgroups)
 * plus the evaluation.  The chain has a slot of its own: a changed grouping, weight, start or plan prepares it again.
 * Refused: whatever cmdgen_multi_pocket_chain or cmdgen_edit_chain refuses - the joint model and no_com_projection handles, group
 * sizes and weights as above, start outside 1 .. timesteps, too few rows of noise, a sample beyond the step's 64 KiB of LDS.
 * Asynchronous on `stream`; cmdgen_chain_status reports this run's checks, drift and NaN resets. */
int cmdgen_multi_edit_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                            int64_t n_groups, const int64_t* group_size_host, const float* weight_host,
                            const float* phar_x, const float* phar_onehot, const float* fix_x, const float* fix_h,
                            int32_t timesteps, int32_t start, int32_t resamplings, int32_t jump_length,
                            const float* noise, int64_t n_draws, uint64_t seed, const int64_t* group_ids_host,
                            float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                            int32_t use_graph, cmdgen_stream stream);

/* Scoring for the CONDITIONAL model (ConditionalDDPM.score): the diffusion loss of a GIVEN pharmacophore in its pocket at a
 * list of noise levels, one evaluation per level, all on the device.  In the normalised space, with xh0 the phar rows and P0
 * the pocket both centred on the phar centre of mass (conditional_model.py:198-320 in eval mode), level k with t = t_levels[k]:
 *   z_k = alpha(t) xh0 + sigma(t) eps_k; (z_k.x, P.x) = remove_mean_batch(z_k.x, P0.x)      (noised_representation)
 *   net = dynamics(z_k, P, t / T)
 *   level_terms_out[k][b][0] = sum over the sample's rows and ALL columns of (eps_k - net)^2   (error_t)
 *   level_terms_out[k][b][1] = the same over the x columns only                               (2 loss_0_x at a t = 0 level)
 *   level_terms_out[k][b][2] = log p(h | z_k) summed over the rows at a t = 0 level, else 0   (-loss_0_h)
 *   level_terms_out[k][b][3] = 1 if the evaluation's velocity was reset by the NaN guard (then net.x = 0 entered the sums), else 0
 *   kl_sums_out[b][0 / 1]    = sum of (alpha_T xh0)^2 over the x / the feature columns         (the two sums of kl_prior)
 * Only raw sums leave the device: the weights 1 - SNR(gamma(t - 1/T) - gamma(t)), T / K, the constants and log p(N) are scalars of
 * (t, n_phar, n_pocket) and the caller assembles nll = loss_t + loss_0 + kl_prior - delta_log_px - log_pN from them
 * (lightning_modules.py:211-229).  Rows are added column by column and then in node index order by one thread (no float atomics):
 * an entry depends on its level's t and draw only, never on the other levels or on how the steps were launched.
 *   phar_x dev [Nl,3], phar_onehot dev [Nl,phar_nf], pocket_x dev [Np,3], pocket_onehot dev [Np,residue_nf]: raw, as
 *          cmdgen_train_noise takes them; copied (normalised) into the handle's buffers before the steps run
 *   t_levels_host int32 [n_levels], each in 0 .. timesteps (any order, repeats allowed; others are refused)
 *   level_coef_host float [n_levels + 1][2] or NULL: (alpha, sigma) of every level and, last, of t = T, as the caller's fp32
 *          evaluation of the schedule gives them (so that they match the reference's torch ops bit for bit); NULL: the library's
 *   noise  dev [n_levels][Nl][3+phar_nf] or NULL: eps_k.  NULL: Philox keyed by (seed, global pocket id) as cmdgen_sample_chain,
 *          with the draw counter k (the index in the list) - cmdgen_debug_noise(seed, id, k, ...) returns the same numbers
 *   level_terms_out dev [n_levels][batch][CMDGEN_SC_COLS], kl_sums_out dev [batch][2]
 * The joint model (its loss has the pocket's own terms) and no_com_projection handles are refused.
 * Asynchronous on `stream`; cmdgen_chain_status reports this run's mean-zero check of every z_k and the levels the NaN guard reset. */
#define CMDGEN_SC_COLS 4
int cmdgen_score_chain(cmdgen_handle* h, const float* phar_x, const float* phar_onehot,
                       const float* pocket_x, const float* pocket_onehot,
                       int32_t n_levels, const int32_t* t_levels_host, const float* level_coef_host,
                       const float* noise, uint64_t seed, const int64_t* pocket_ids_host,
                       float* level_terms_out, float* kl_sums_out, int32_t use_graph, cmdgen_stream stream);

/* Scoring ONE pharmacophore against SEVERAL pockets (ConditionalDDPM.score_given_pockets): the variational bound of the sampler that
 * cmdgen_multi_pocket_chain runs, whose denoiser is eps_bar = sum_m w_m eps_m - cmdgen_score_chain's levels with eps_bar in place of
 * net.  Layout, groups, weights and group_ids_host are exactly cmdgen_multi_pocket_chain's (B member samples, the members of a group
 * consecutive, Nu = one copy of the phar rows per group, the pockets of a group in ONE common frame); levels, level_coef_host and the
 * output columns are exactly cmdgen_score_chain's.  In the normalised space, for group g with the clean rows xh0_g and the pockets
 * P0_m of its members, all centred on the centre of mass of the group's phar rows (summed from the raw input in index order), level
 * k with t = t_levels[k] and ONE draw eps_k per group:
 *   z_k = alpha(t) xh0_g + sigma(t) eps_k;  shift = com(z_k.x);  z_k.x -= shift;  P_m.x = P0_m.x - shift for every member
 *   eps_m = dynamics(z_k, P_m, t / T): the ordinary evaluation over the B member samples (x columns zero under the batch-wide NaN guard)
 *   eps_bar = sum_m w_m eps_m                (m ascending, the first term not added to a zero)
 *   group_terms_out[k][g]  = the CMDGEN_SC_COLS columns of cmdgen_score_chain with eps_bar in place of net
 *   member_terms_out[k][b] = the same columns with member b's own eps_b: what cmdgen_score_chain gives on the member layout when every
 *                            member gets its group's rows and draws - the per-pocket scores on COMMON draws
 *   kl_sums_out[g][0 / 1]  = cmdgen_score_chain's two sums on xh0_g
 * Rows are added column by column and then in node index order by one thread, no float atomics.  With every M_g = 1 every value is
 * cmdgen_score_chain's, bit for bit.
 *   phar_x dev [Nu,3], phar_onehot dev [Nu,phar_nf]: raw, one row per unique phar row;  pocket_x dev [Np,3], pocket_onehot dev
 *          [Np,residue_nf]: raw, the rows of the B member samples in layout order
 *   n_groups, group_size_host, weight_host  as cmdgen_multi_pocket_chain
 *   n_levels, t_levels_host, level_coef_host  as cmdgen_score_chain
 *   noise  dev [n_levels][Nu][3+phar_nf] or NULL: eps_k, one draw per group and level.  NULL: Philox keyed by (seed, global GROUP id,
 *          level index k, node of the group) - cmdgen_debug_noise(seed, group id, k, n_phar, ...) returns the same numbers
 *   group_ids_host  host [n_groups] global group ids for the Philox key (NULL: 0 .. n_groups-1)
 *   group_terms_out dev [n_levels][n_groups][CMDGEN_SC_COLS];  member_terms_out dev [n_levels][batch][CMDGEN_SC_COLS] or NULL;
 *   kl_sums_out dev [n_groups][2]
 * One level is one launch (k_multi_score_step: one workgroup per member, each with its own copy of the clean rows and of z - no float
 * atomics, no synchronisation between workgroups) plus the evaluation.  The chain has a slot of its own: a changed level list,
 * grouping or weight prepares it again; the caller's pointers are the graph key.
 * Refused: whatever cmdgen_multi_pocket_chain refuses of a grouping (sizes, unequal n_phar in a group, weights) and cmdgen_score_chain of
 * a level list (levels outside 0 .. timesteps, n_levels < 1, a sample beyond the step's 64 KiB of LDS), the joint model,
 * no_com_projection handles and null pointers.
 * Asynchronous on `stream`; cmdgen_chain_status reports this run's mean-zero check of every z_k and the levels the NaN guard reset;
 * cmdgen_debug_read("chain_z") gives every member's copy of the last level's z. */
int cmdgen_multi_score_chain(cmdgen_handle* h, const float* phar_x, const float* phar_onehot,
                             const float* pocket_x, const float* pocket_onehot,
                             int64_t n_groups, const int64_t* group_size_host, const float* weight_host,
                             int32_t n_levels, const int32_t* t_levels_host, const float* level_coef_host,
                             const float* noise, uint64_t seed, const int64_t* group_ids_host,
                             float* group_terms_out, float* member_terms_out, float* kl_sums_out,
                             int32_t use_graph, cmdgen_stream stream);

/* Sampling steered by geometric restraints (ConditionalDDPM.sample_restrained): cmdgen_sample_chain's chain - the same ops, draws and
 * Philox counters - with one addition to the mean of every posterior op t -> s (classifier guidance); the decode op is not guided.
 * The definition is the project's own (the reference has nothing like it); kernels_restrain.hip carries it in full.  Per sample and op,
 * with z the op's input, e the network's x columns after the NaN guard, P the current (translated, normalised) pocket, P_in the caller's
 * pocket, n_x = norm_values[0] and coef the op's step-table row:
 *   xhat_i = n_x (z.x_i - sigma_t e_i) / alpha_t             the denoised estimate, in Angstrom, in the chain's current frame
 *   shift  = n_x (com(P.x) - com(P_in.x / n_x))              centres c of the caller's frame become c + shift; q_a = n_x P.x_a
 *   E      = sum over restraints of 0.5 k v^2                v >= 0 the violation in Angstrom, k >= 0 in 1/Angstrom^2:
 *            position(point i, c, r, k)   v = max(0, |xhat_i - (c + shift)| - r)
 *            distance(points i, j, lo, hi, k)  v = max(0, lo - d, d - hi), d = |xhat_i - xhat_j|
 *            exclusion(c, r, k)           for every point of the sample  v_i = max(0, r - |xhat_i - (c + shift)|)
 *            clash(r_c, k_c)              for every point and pocket atom of every sample  v_ia = max(0, r_c - |xhat_i - q_a|)
 *   g_i    = dE / dxhat_i                                     (a term whose distance is below 1e-12 A contributes the zero vector)
 *   d_i    = -scale (n_x coef.z)^2 g_i,  scaled down to |d_i| = max_shift when longer;  d = 0 for an op with t / T > guide_below
 *   mu.x_i = z.x_i / coef.x - coef.y e_i + d_i / n_x          the h columns, the draw, the projection and the saved steps as before
 * sigma_t and alpha_t come from the guide table (cmdgen_set_guide_table, or the library's own evaluation of the gamma table).
 * With no restraint on any sample and clash_radius = 0, or with scale = 0, every output equals cmdgen_sample_chain's bit for bit; a
 * sample that no restraint touches takes k_step_count's arithmetic.  No float atomics: two runs of the same inputs are equal bit for bit.
 *   restraints_host  host [n_restraints] (or NULL with n_restraints = 0), any order; a sample's restraints keep their list order
 *   clash_radius, clash_k   r_c in Angstrom (0: off), k_c
 *   scale, max_shift (Angstrom, > 0), guide_below in [0, 1]
 *   energy_out     dev [batch][2]: E and the largest violation (Angstrom) of the RETURNED xh_phar / xh_pocket, shift taken from the
 *                  returned pocket
 *   op_energy_out  dev [K][batch] E at xhat of every op, or NULL
 *   the other arguments as cmdgen_sample_chain
 * The chain has a slot of its own and is captured like the others; the restraint table and the five scalars are part of the slot's
 * tables, so a change prepares the slot (and its graph) again.
 * Refused (CMDGEN_EINVAL): an unknown kind, a sample index outside the layout, a point index >= n_phar of its sample, i == j, lo > hi,
 * a negative or non-finite radius, bound, centre, k, scale or clash value, max_shift <= 0, guide_below outside [0, 1], more than
 * CMDGEN_MAX_RESTRAINTS restraints on one sample, a sample beyond the step's 64 KiB of LDS, a no_com_projection handle; the joint
 * model (CMDGEN_ESTATE).
 * Asynchronous on `stream`; cmdgen_chain_status reports this run's checks, drift and NaN resets. */
#define CMDGEN_RESTRAINT_POSITION  0
#define CMDGEN_RESTRAINT_DISTANCE  1
#define CMDGEN_RESTRAINT_EXCLUSION 2
#define CMDGEN_MAX_RESTRAINTS 256      /* per sample */
typedef struct {
    int32_t kind, sample, i, j;        /* position: point i; distance: points i, j; exclusion: neither */
    float c[3], a, b, k;               /* centre; a, b: radius, - | lo, hi | radius, -; k */
} cmdgen_restraint;
int cmdgen_restrained_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot, int32_t timesteps,
                            const cmdgen_restraint* restraints_host, int64_t n_restraints,
                            float clash_radius, float clash_k, float scale, float max_shift, float guide_below,
                            const float* noise, uint64_t seed, const int64_t* pocket_ids_host,
                            float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                            float* energy_out, float* op_energy_out, int32_t use_graph, cmdgen_stream stream);

/* Editing under restraints (ConditionalDDPM.edit_restrained): cmdgen_edit_chain's chain - the same init (from the prior, or z ~ q(z_start | K)
 * when start < timesteps), op table, draws and Philox counters, B merge, C jump, saved steps and decode - with cmdgen_restrained_chain's
 * guidance in the mean of op A of every op t -> s.  The definition is the project's own; kernels_restrain.hip (k_restrained_edit_step_count)
 * carries it in full.  The terms, the shift, g_i, d_i and mu are cmdgen_restrained_chain's, with three points settled:
 *   xhat_i  of a row whose x columns are not held is the restrained chain's; of a row whose x columns ARE held it is n_x K_i.x + shift, its
 *           given position moved into the current frame as a restraint centre is (K the normalised given rows) - a distance restraint
 *           between a free and a held point pulls toward the true held position
 *   d_i     is added to the mean of rows whose x is not held; a row whose x is held gets nothing added, not even a zero (B replaces it),
 *           while its energy terms still count in E.  A row with only its types held is a free row here
 *   sigma_t, alpha_t  one row per op of the edit plan (n_steps, following the plan's s with its repeats after jumps): the op that goes to
 *           level s takes row K - 1 - s of the guide table (cmdgen_set_guide_table with K = timesteps, or the library's own evaluation).
 *           Op C and the decode are never guided
 * Reductions that hold bit for bit on every output, cmdgen_chain_status and cmdgen_debug_read("chain_z"):
 *   - no restraint on any sample and clash_radius = 0, or scale = 0: cmdgen_edit_chain's outputs for the same arguments (start < timesteps,
 *     resamplings > 1 and jump_length > 1 included)
 *   - no mark in either mask, start = timesteps, resamplings = jump_length = 1: cmdgen_restrained_chain's outputs on a handle whose
 *     evaluations use their own k_readout (option readout_in_coord = 0), energy_out, op_energy_out, z_steps and pocket_steps included
 *     (noise rows in cmdgen_edit_chain's order)
 *   - a sample that no restraint touches and an op above guide_below run cmdgen_edit_chain's arithmetic
 *   - two runs of the same inputs are equal bit for bit (no float atomics)
 *   energy_out     dev [batch][2]: E and the largest violation (Angstrom) of the RETURNED rows, held points included at their returned positions
 *   op_energy_out  dev [n_steps][batch] E at xhat of every op (n_steps of cmdgen_edit_plan), or NULL
 *   the other arguments as cmdgen_edit_chain, then as cmdgen_restrained_chain; cmdgen_edit_plan gives n_steps and n_draws
 * The chain has a slot of its own; the plan's tables, the guide rows, the five scalars and the restraint table are the slot's tables, so a
 * changed plan, start, restraint or scalar prepares the slot (and its graph) again.
 * Refused: whatever cmdgen_edit_chain or cmdgen_restrained_chain refuses, with the same codes. */
int cmdgen_restrained_edit_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                 const float* phar_x, const float* phar_onehot, const float* fix_x, const float* fix_h,
                                 int32_t timesteps, int32_t start, int32_t resamplings, int32_t jump_length,
                                 const float* noise, int64_t n_draws, uint64_t seed, const int64_t* pocket_ids_host,
                                 float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                 const cmdgen_restraint* restraints_host, int64_t n_restraints,
                                 float clash_radius, float clash_k, float scale, float max_shift, float guide_below,
                                 float* energy_out, float* op_energy_out, int32_t use_graph, cmdgen_stream stream);

/* Restraints on the shared latent of several pockets (ConditionalDDPM.sample_restrained_given_pockets): cmdgen_multi_pocket_chain's chain -
 * the same layout of B member samples in G groups, the same init, ops, draws, Philox counters (keyed by group id), decode and CoG
 * re-centring - with cmdgen_restrained_chain's addition to the mean of every posterior op t -> s, applied PER GROUP.  The decode is not
 * guided.  The definition is the project's own; kernels_restrain.hip ("The restrained MULTI-POCKET chain") carries it in full.  The terms,
 * g_i, d_i, the max_shift clip, guide_below and mu are cmdgen_restrained_chain's, with these points settled:
 *   restraints  belong to a GROUP: cmdgen_restraint::sample is the group index g, point indices are < n_phar of the group, centres are
 *               given in the common frame in which the caller gives the group's pockets
 *   xhat_i      = n_x (z.x_i - sigma_t ebar_i) / alpha_t with ebar = sum_m w_m eps_m, what the step itself uses (m ascending, the first
 *               term not added to a zero); its x columns are zero under the batch-wide NaN guard
 *   shift_g     = n_x (com(P_first.x) - com(P_first,in.x / n_x)), from the group's FIRST member, its pocket as it stands at the op's input:
 *               the precedent of cmdgen_multi_edit_chain, whose offset in step B is the first member's
 *   clash       the sum runs over every point of the group and every pocket atom of EVERY member, q_{m,a} = n_x P_m.x_a as it stands at the
 *               op's input; unweighted, weight-0 members included: a point must clash with neither pocket
 *   sums        a point's terms: the group's records and the first member's atoms as cmdgen_restrained_chain sums them, then the further
 *               members' atoms, member by member in ascending order; a fixed order, no float atomics
 *   mu.x_i      = z.x_i / coef.x - coef.y ebar_i + d_i / n_x: every member adds the SAME BITS d_i, so the members' copies of z stay
 *               bit-identical (cmdgen_debug_read("chain_z"))
 * Reductions that hold bit for bit on every output and cmdgen_chain_status:
 *   - no record on any group and clash_radius = 0, or scale = 0, or guide_below = 0: cmdgen_multi_pocket_chain's outputs; a group-op that
 *     is not guided (no record on the group while clash_radius = 0, scale = 0, t / T > guide_below) adds nothing, not even a zero
 *   - every group of one member: cmdgen_restrained_chain's outputs on a handle whose evaluations use their own k_readout (option
 *     readout_in_coord = 0), energy_out and op_energy_out included
 *   - two runs of the same inputs are equal bit for bit, captured or eager
 *   energy_out     dev [G][2]: E and the largest violation (Angstrom) of the RETURNED rows against every member's returned pocket, the
 *                  shift taken from the first member's returned pocket
 *   op_energy_out  dev [K][G] E at xhat of every op, or NULL
 *   the leading arguments as cmdgen_multi_pocket_chain, the restraint arguments as cmdgen_restrained_chain, then cmdgen_multi_pocket_chain's
 * The chain has a slot of its own; its tables are the posterior rows, the group tables and the guidance tail (CSR offsets [G + 1]), so a
 * changed grouping, weight, restraint or scalar prepares the slot (and its graph) again.
 * Refused: whatever cmdgen_multi_pocket_chain refuses of a grouping and whatever cmdgen_restrained_chain refuses of a restraint list and
 * scalars, with the same codes; the messages say "group" where a group is meant.  The joint model and no_com_projection handles
 * (CMDGEN_ESTATE, as cmdgen_multi_pocket_chain). */
int cmdgen_multi_restrained_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                  int64_t n_groups, const int64_t* group_size_host, const float* weight_host, int32_t timesteps,
                                  const cmdgen_restraint* restraints_host, int64_t n_restraints,
                                  float clash_radius, float clash_k, float scale, float max_shift, float guide_below,
                                  const float* noise, uint64_t seed, const int64_t* group_ids_host,
                                  float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                  float* energy_out, float* op_energy_out, int32_t use_graph, cmdgen_stream stream);

/* Editing under restraints for several pockets (ConditionalDDPM.edit_restrained_given_pockets): all three modifiers at once.  The chain is
 * cmdgen_multi_edit_chain's - the same layout of B member samples in G groups, both inits, the plan, the op table, the draw rows and the
 * Philox counters keyed by group id, the B merge with the group's offset, the C jump, the saved steps, the decode and the CoG re-centring -
 * with cmdgen_multi_restrained_chain's guidance in the mean of op A of every op t -> s, once per GROUP.  The definition is the project's
 * own; kernels_restrain.hip ("The restrained MULTI-POCKET EDIT chain") carries it in full.  The terms, the clash over every member's atoms,
 * the order of the sums, the max_shift clip and guide_below are cmdgen_multi_restrained_chain's, with three points settled as
 * cmdgen_restrained_edit_chain settles them:
 *   xhat_i   of a row of the group whose x columns are not held is n_x (z.x_i - sigma_t ebar_i) / alpha_t, ebar = sum_m w_m eps_m (m ascending,
 *            the first term not added to a zero; zero x columns under the batch-wide NaN guard); of a row whose x columns ARE held (fix_x of
 *            the group's row non-zero) it is n_x K_i.x + shift_g, its given position moved into the current frame as a restraint centre is
 *   shift_g  = n_x (com(P_first.x) - com(P_first,in.x / n_x)), from the group's FIRST member, its pocket as it stands at the op's input -
 *            which also covers start < timesteps, where the init has re-centred every pocket on the given rows' centre.  Step B keeps its
 *            own offset, as in cmdgen_multi_edit_chain
 *   mu.x_i   = z.x_i / coef.x - coef.y ebar_i + d_i / n_x on rows whose x is not held; a row whose x is held gets nothing added, not even a
 *            zero (B replaces it), while its energy terms still count in E and op_energy.  A row with only its types held is a free row
 *            here.  Every member adds the SAME BITS d_i, so the members' copies of z stay bit-identical (cmdgen_debug_read("chain_z"))
 *   sigma_t, alpha_t  one row per op of the edit plan (n_steps, repeats after jumps included): the op that goes to level s takes row
 *            K - 1 - s of the guide table (cmdgen_set_guide_table with K = timesteps, or the library's own evaluation).  Op C and the
 *            decode are never guided
 * Reductions that hold bit for bit on every output, cmdgen_chain_status and cmdgen_debug_read("chain_z"):
 *   - no record on any group and clash_radius = 0, or scale = 0, or guide_below = 0: cmdgen_multi_edit_chain's outputs for the same
 *     arguments (start < timesteps, resamplings > 1 and jump_length > 1 included); a group-op that is not guided adds nothing, not even a zero
 *   - every group of one member: cmdgen_restrained_edit_chain's outputs, energy_out and op_energy_out included, with no option set
 *   - no mark in either mask, start = timesteps, resamplings = jump_length = 1: cmdgen_multi_restrained_chain's outputs (noise rows in
 *     cmdgen_multi_edit_chain's order)
 *   - two runs of the same inputs are equal bit for bit, captured or eager (no float atomics)
 *   energy_out     dev [G][2]: E and the largest violation (Angstrom) of the RETURNED rows, held points included at their returned positions,
 *                  against every member's returned pocket, the shift taken from the first member's returned pocket
 *   op_energy_out  dev [n_steps][G] E at xhat of every op (n_steps of cmdgen_edit_plan), or NULL
 *   the other arguments as cmdgen_multi_edit_chain, then as cmdgen_multi_restrained_chain (cmdgen_restraint::sample is the GROUP index);
 *   cmdgen_edit_plan gives n_steps and n_draws; injected noise is [n_draws][Nu][3 + phar_nf]
 * The chain has a slot of its own; its tables are the edit plan's tables, the group tables and the guidance tail (one guide row per op of
 * the plan, the five scalars, CSR offsets [G + 1], the records sorted by group), so a changed grouping, weight, plan, start, restraint or
 * scalar prepares the slot (and its graph) again.
 * Refused: whatever cmdgen_multi_edit_chain refuses and whatever cmdgen_multi_restrained_chain refuses of a restraint list and scalars,
 * with the same codes; the messages name the argument and say "group" where a group is meant.  The joint model and no_com_projection
 * handles (CMDGEN_ESTATE). */
int cmdgen_multi_restrained_edit_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                       int64_t n_groups, const int64_t* group_size_host, const float* weight_host,
                                       const float* phar_x, const float* phar_onehot, const float* fix_x, const float* fix_h,
                                       int32_t timesteps, int32_t start, int32_t resamplings, int32_t jump_length,
                                       const float* noise, int64_t n_draws, uint64_t seed, const int64_t* group_ids_host,
                                       float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                       const cmdgen_restraint* restraints_host, int64_t n_restraints,
                                       float clash_radius, float clash_k, float scale, float max_shift, float guide_below,
                                       float* energy_out /* dev [G][2] */, float* op_energy_out /* dev [n_steps][G] or NULL */,
                                       int32_t use_graph, cmdgen_stream stream);

/* ---- diverse sampling: push apart the samples drawn for one pocket ---------------------- */
/* cmdgen_sample_chain's chain (the same init, ops, draws, Philox counters keyed by pocket_ids, saved steps, decode and CoG fix; the
 * evaluations run their own k_readout) with a term in the mean of every posterior op that couples the samples of a SET: particle guidance
 * (Corso et al., 2023).  The reference draws independently and has nothing like it; the definition is the project's (the header of
 * csrc/kernels_diverse.hip; INTEGRATION.md, "Diverse sampling").
 *   Sets.  The layout's B samples are partitioned into n_sets sets of consecutive samples (set_size_host, every size >= 1, summing to B): "the
 *     draws for one pocket".  Members may have different numbers of points.  The library does not check that the members' pockets are copies
 *     of each other: positions are compared in the frame in which the caller gives each sample's pocket.
 *   With z, e (zero under the NaN guard), P, P_in, n_x, coef and the guide row (sigma_t, alpha_t) as for cmdgen_restrained_chain, w = width
 *   (A), k = strength (dimensionless) and M_a the size of sample a's set, at every posterior op t -> s:
 *   1. xhat_ai = n_x (z.x_ai - sigma_t e_ai) / alpha_t;  shift_a = n_x (com(P_a.x) - com(P_a,in.x / n_x));  y_ai = xhat_ai - shift_a.
 *   2. o_ai = (1 / (M_a - 1)) sum_{b != a, same set} sum_j exp(-|y_ai - y_bj|^2 / (2 w^2)), overlap_a = sum_i o_ai.  The set's energy is
 *      E = k / (M - 1) sum_{a < b} sum_{i, j} exp(.) and g_ai = -(k / ((M_a - 1) w^2)) sum_{b != a} sum_j exp(.) (y_ai - y_bj).
 *   3. d_ai = -(n_x coef.z)^2 g_ai (A), scaled back to max_shift when longer.  An op with t / T > guide_below, a sample with M_a = 1 and a
 *      call with k = 0 have no displacement: nothing is added, not even a zero.
 *   4. mu.x_ai = z.x_ai / coef.x - coef.y e_ai + d_ai / n_x; everything else is the plain step's.  The decode is not guided.
 *   overlap_out  dev [B]: step 2 on the RETURNED rows, shift_a = com(xh_pocket_out_a.x) - n_x com(P_a,in.x / n_x); 0 where M_a = 1.
 *   op_overlap_out  dev [K][B] or NULL: step 2 at every op's estimate, also when k = 0 or the op is above guide_below.
 *   the other arguments as cmdgen_sample_chain; cmdgen_set_guide_table supplies (sigma_t, alpha_t) as for cmdgen_restrained_chain.
 * Sums run in a fixed order without float atomics: two runs are equal bit for bit, captured or eager.  k = 0, guide_below = 0 and sets of one
 * member each give cmdgen_sample_chain's outputs bit for bit (on a handle with readout_in_coord = 0); overlap_out is still reported under k = 0.
 * The chain has a slot of its own; the guide rows, the scalars and the set tables are part of its table block, so a changed partition or
 * scalar prepares the slot (and its graph) again.
 * Refused with CMDGEN_EINVAL, nothing launched: null pointers, n_sets outside [1, B], a set size below 1, sizes that do not sum to B, strength
 * non-finite or negative, width non-finite or <= 0, max_shift <= 0, guide_below outside [0, 1], a set with more than CMDGEN_MAX_SET_ROWS phar
 * rows (a capacity cap: the pair launch costs rows^2), a sample beyond the step's 64 KiB of LDS, a no_com_projection handle; the joint model
 * (CMDGEN_ESTATE). */
#define CMDGEN_MAX_SET_ROWS 8192
int cmdgen_diverse_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot, int32_t timesteps,
                         int64_t n_sets, const int64_t* set_size_host,
                         float strength, float width, float max_shift, float guide_below,
                         const float* noise, uint64_t seed, const int64_t* pocket_ids_host,
                         float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                         float* overlap_out /* dev [B] */, float* op_overlap_out /* dev [K][B] or NULL */,
                         int32_t use_graph, cmdgen_stream stream);

/* ---- diverse sampling under restraints: both terms in one chain ------------------------- */
/* cmdgen_sample_chain's chain (the same init, ops, draws, Philox counters keyed by pocket_ids, saved steps and CoG fix; the decode is
 * unguided; the evaluations run their own k_readout, there is no own-velocity form) with BOTH steering terms in the mean of every posterior
 * op t -> s (the header of k_diverse_restrained_step_count in csrc/kernels_restrain.hip; INTEGRATION.md, "Diverse sampling under
 * restraints").  Both are taken at the same point, the denoised estimate of the op's input; each keeps the definition and the scalars of its
 * own chain:
 *   1. Restraint term.  Steps 1-4 of cmdgen_restrained_chain give d^r_i = -scale (n_x coef.z)^2 g_i from the sample's records and the clash
 *      pair, clipped at max_shift.  Active for a touched sample (a record on it, or clash_radius > 0) when scale > 0 and t / T <= guide_below.
 *   2. Overlap term.  Steps 1-3 of cmdgen_diverse_chain give d^v_ai from the set's y = xhat - shift with strength and width, clipped at its
 *      own diverse_max_shift.  Active for a sample of a set with M > 1 when strength > 0 and t / T <= diverse_guide_below.
 *   3. mu.x_i = ((z.x_i / coef.x - coef.y e_i) + d^r_i / n_x) + d^v_i / n_x: the two additions in that order, each made only where its term
 *      is active; nothing is added for an inactive term, not even a zero.  Everything else is the plain step's.
 *   energy_out dev [B][2] and op_energy_out dev [K][B] or NULL exactly as cmdgen_restrained_chain reports them; overlap_out dev [B] and
 *   op_overlap_out dev [K][B] or NULL exactly as cmdgen_diverse_chain reports them (a per-op output is still computed where its term is
 *   inactive but defined).  The other arguments as the two parents'; cmdgen_set_guide_table supplies (sigma_t, alpha_t) for both terms.
 * Reductions that hold bit for bit on every output and the chain status, on a handle with readout_in_coord = 0:
 *   strength = 0, or diverse_guide_below = 0, or every set of one member: cmdgen_restrained_chain's outputs, energy and op_energy included;
 *   scale = 0, or no record and clash_radius = 0: cmdgen_diverse_chain's outputs, overlap and op_overlap included;
 *   both at once: cmdgen_sample_chain's outputs.
 * Sums are the parents' (a fixed order, no float atomics): two runs are equal bit for bit, captured or eager.  The chain has a slot of its
 * own; the records, the partition and the scalars of both parts are part of its table block, so a change of any prepares the slot (and its
 * graph) again.
 * Refused with CMDGEN_EINVAL, nothing launched: what either parent refuses of its own arguments, in the parent's words; a sample beyond the
 * step's 64 KiB of LDS (92 B per node at phar_nf 8: more than 712 nodes, where cmdgen_diverse_chain takes 1024); a no_com_projection handle;
 * the joint model (CMDGEN_ESTATE).  Not combined with groups or given rows. */
int cmdgen_diverse_restrained_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot, int32_t timesteps,
                                    const cmdgen_restraint* restraints_host, int64_t n_restraints,
                                    float clash_radius, float clash_k, float scale, float max_shift, float guide_below,
                                    int64_t n_sets, const int64_t* set_size_host,
                                    float strength, float width, float diverse_max_shift, float diverse_guide_below,
                                    const float* noise, uint64_t seed, const int64_t* pocket_ids_host,
                                    float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                    float* energy_out /* dev [B][2] */, float* op_energy_out /* dev [K][B] or NULL */,
                                    float* overlap_out /* dev [B] */, float* op_overlap_out /* dev [K][B] or NULL */,
                                    int32_t use_graph, cmdgen_stream stream);

/* ---- training step (conditional model) -------------------------------------------------- */
/* The trainable tensors of EGNNDynamics live in ONE flat fp32 device buffer owned by the caller, in the
 * reference's registration order (the state_dict order below 'ddpm.dynamics.': weight then bias of every
 * nn.Linear, dynamics.py:21-60, egnn_new.py:15-29, :78-83) - so that the gradient is one contiguous bucket
 * (a single RCCL all-reduce per step replaces DDP's bucketing, train.py:111-121) and the optimizer is one
 * elementwise kernel.  Every tensor starts on a 16-byte boundary (a few zero padding floats in between).
 * cmdgen_param_count (buffer length incl. padding) / cmdgen_param_offset describe the layout
 * (name e.g. "egnn.e_block_0.gcl_0.edge_mlp.0.weight"). */
int cmdgen_param_count(cmdgen_handle* h, int64_t* n_params);
int cmdgen_param_offset(cmdgen_handle* h, const char* name, int64_t* offset, int64_t* count);

/* EGNNDynamics.forward (dynamics.py:75-139) on the parameters `theta`, keeping every activation the backward
 * pass needs (after cmdgen_set_layout; no cmdgen_finalize_weights needed).  t dev [batch].  Writes
 * eps_phar dev [Nl, 3+phar_nf] and, when non-NULL, eps_pocket dev [Np, 3+residue_nf] (required for the joint model,
 * config.update_pocket_coords = 1; the conditional loss never uses it).  Waits once for the host copy of the two list lengths (they
 * size the activation store and the grids; the parameter re-packs are queued behind that copy, so the device keeps working while the
 * host wakes up). */
int cmdgen_train_forward(cmdgen_handle* h, const float* theta, const float* xh_phar, const float* xh_pocket,
                         const float* t, float* eps_phar, float* eps_pocket, cmdgen_stream stream);

/* Backward of the last cmdgen_train_forward: given dL/d eps_phar (dev [Nl, 3+phar_nf]) and optionally
 * dL/d eps_pocket (dev [Np, 3+residue_nf], NULL = zero) ADDS dL/d theta into
 * `grad` (dev, same layout as theta; zero it first for a fresh gradient).  What autograd does for
 * loss.backward() in the reference's training_step (lightning_modules.py:245-260).
 * Streams: the pass queues its weight / bias gradients on streams of the handle beside the chain of data gradients it queues on `stream`
 * (option "wgrad_stream"); before the call returns, `stream` has been made to wait for all of them - work queued on `stream` after the
 * call (the optimizer, an all-reduce ordered behind `stream`) sees the complete gradient, exactly as if everything had run on `stream`.
 * Gradients are accumulated with float atomics: equal run to run up to the order of those sums. */
int cmdgen_train_backward(cmdgen_handle* h, const float* d_eps_phar, const float* d_eps_pocket, float* grad,
                          cmdgen_stream stream);

/* The same pass in stages, so that the gradient all-reduce of the blocks already differentiated overlaps the rest of
 * the backward pass (DDP's bucketed overlap, train.py:111-121): stage 0 = readout, stage k in 1..n_layers = block
 * n_layers-k, stage n_layers+1 = embedding and encoders.  Call with consecutive, ascending stage ranges covering
 * 0..n_layers+1; after stage k the flat gradient is final from cmdgen_param_offset("egnn.e_block_<n_layers-k>.
 * gcl_0.edge_mlp.0.weight") to its end. */
int cmdgen_train_backward_stages(cmdgen_handle* h, const float* d_eps_phar, const float* d_eps_pocket, float* grad,
                                 int32_t first_stage, int32_t last_stage, cmdgen_stream stream);

/* The backward pass of the last cmdgen_train_forward to its INPUTS as well as to the parameters: the reference's autograd
 * gradients of EGNNDynamics.forward (dynamics.py:75-139) with respect to xh_phar, xh_pocket and t.  grad (may be NULL: no
 * parameter gradient is wanted) is accumulated exactly as cmdgen_train_backward accumulates it; the input gradients are
 * WRITTEN (not accumulated), each only where its pointer is non-NULL:
 *   d_xh_phar [Nl,3+phar_nf], d_xh_pocket [Np,3+residue_nf]: position columns through every radial, coord_diff and d0
 *     term of every row (pocket rows that do not move included), the direct term of vel = x_final - x (and its centre-of-mass
 *     projection when update_pocket_coords; zero where the NaN guard reset vel), feature columns through the encoders;
 *   d_t [batch]: per-sample sum of the time column (condition_time; refused without it).
 * The radius graph is a constant of the pass (as in the reference, whose edge set carries no gradient).  After a NaN reset of
 * the forward's velocity (dynamics.py:129-131) no gradient flows through vel.  Any evaluation, chain or new layout on the handle
 * since the forward replaces the graph the pass reads: the call then fails with CMDGEN_ESTATE (run the forward again;
 * cmdgen_query "eval_gen" counts such calls).  The call changes nothing cmdgen_train_backward does: same kernels, same
 * parameter gradient (both up to the order of float atomics). */
int cmdgen_train_backward_inputs(cmdgen_handle* h, const float* d_eps_phar, const float* d_eps_pocket, float* grad,
                                 float* d_xh_phar, float* d_xh_pocket, float* d_t, cmdgen_stream stream);

/* The loss side of ConditionalDDPM.forward in training mode (conditional_model.py:198-320) and of
 * PharPocketDDPM.forward (lightning_modules.py:188-239), fused: three launches per step instead of a few hundred
 * small tensor operations.  Per-sample scalars that depend only on t and on the node counts are made by the host
 * and passed as `tab`, dev, COLUMN-major [CMDGEN_TT_COLS][batch]:
 *   0 alpha_t, 1 sigma_t, 2 t_is_zero, 3 SNR weight 1 - SNR(gamma_s - gamma_t), 4 alpha_T, 5 sigma_T,
 *   6 -log_constants_p_x_given_z0, 7 delta_log_px, 8 log p(N), 9 t_int, 10 t = t_int / T (column 10 is the `t`
 *   argument of cmdgen_train_forward), 11 sigma_t * norm_values[1].
 * cmdgen_train_noise: normalize + remove_mean_batch + noised_representation (conditional_model.py:80-106, :467-475; on a handle
 *   configured with no_com_projection - SimpleConditionalDDPM, :481-525 - the pocket's centre of mass is subtracted instead and nothing
 *   is projected, and the caller's `tab` counts n_phar * 3 degrees of freedom):
 *   from the raw batch (phar_x [Nl,3], phar_one_hot [Nl,phar_nf], pocket_x [Np,3], pocket_one_hot [Np,residue_nf]) and the
 *   Gaussian draw eps [Nl,3+phar_nf] writes z_t [Nl,3+phar_nf], xh_pocket [Np,3+residue_nf] (the network's inputs) and
 *   kl_sums [batch,2] (sum of (alpha_T x)^2 and (alpha_T h)^2 of the clean sample, for kl_prior, :49-59).
 * cmdgen_train_loss: from net_out = eps_phar of cmdgen_train_forward writes
 *   terms [batch, CMDGEN_TS_COLS]: 0 nll, 1 error_t (as logged), 2 loss_0, 3 kl_prior, 4 / 5 mean |eps_hat| of x / h,
 *   6 loss_0_x, 7 loss_0_h, 8 loss_t;   means [CMDGEN_TS_COLS] = their batch means (means[0] is the loss);
 *   d_eps [Nl,3+phar_nf] = d loss / d net_out, the input of cmdgen_train_backward.
 *   l2 != 0: loss_type 'l2' (lightning_modules.py:198-205); 0: the vlb weighting (:206-212) with T diffusion steps. */
#define CMDGEN_TT_COLS 12
#define CMDGEN_TS_COLS 12
int cmdgen_train_noise(cmdgen_handle* h, const float* phar_x, const float* phar_one_hot, const float* pocket_x,
                       const float* pocket_one_hot, const float* tab, const float* eps, float* z_t, float* xh_pocket,
                       float* kl_sums, cmdgen_stream stream);
int cmdgen_train_loss(cmdgen_handle* h, int32_t l2, float T, const float* net_out, const float* eps, const float* z_t,
                      const float* phar_one_hot, const float* tab, const float* kl_sums, float* terms, float* d_eps,
                      float* means, cmdgen_stream stream);

/* The same two launches for the JOINT model (mode 'joint': EnVariationalDiffusion.forward in training mode, en_diffusion.py:332-465,
 * with the joint branch of lightning_modules.py:198-217): the pocket is noised and denoised too.  `tab` as above with the node count
 * n_phar + n_pocket in columns 6 and 7 and the JOINT log p(n_phar, n_pocket) in column 8.
 * cmdgen_train_noise_joint: draw_phar [Nl,3+phar_nf] / draw_pocket [Np,3+residue_nf] are raw Gaussian draws; writes eps_phar / eps_pocket
 *   (the draws with the x-part's centre of mass over all nodes of the sample removed, :555-574), z_phar / z_pocket = alpha_t xh +
 *   sigma_t eps (the network's inputs) and kl_sums [batch,2] over both parts.
 * cmdgen_train_loss_joint: net_phar / net_pocket = both outputs of cmdgen_train_forward; terms columns 0..8 as above (1, 4, 5 for the
 *   phar part; 6 = loss_0_x of both parts), 9 error_t of the pocket part, 10 / 11 mean |eps_hat| of the pocket's x / h;
 *   d_eps_phar / d_eps_pocket = d loss / d net outputs, the inputs of cmdgen_train_backward. */
int cmdgen_train_noise_joint(cmdgen_handle* h, const float* phar_x, const float* phar_one_hot, const float* pocket_x,
                             const float* pocket_one_hot, const float* tab, const float* draw_phar, const float* draw_pocket,
                             float* z_phar, float* z_pocket, float* eps_phar, float* eps_pocket, float* kl_sums, cmdgen_stream stream);
int cmdgen_train_loss_joint(cmdgen_handle* h, int32_t l2, float T, const float* net_phar, const float* net_pocket,
                            const float* eps_phar, const float* eps_pocket, const float* z_phar, const float* z_pocket,
                            const float* phar_one_hot, const float* pocket_one_hot, const float* tab, const float* kl_sums,
                            float* terms, float* d_eps_phar, float* d_eps_pocket, float* means, cmdgen_stream stream);

/* GEMM operand precision of the training step's backward products: 0 (default) = fp32 results (fp32-accurate split-bf16
 * products or, with cmdgen_set_gemm_mode(0), the fp32 matrix instruction), 1 = operands rounded to bf16 (nearest-even),
 * fp32 accumulation on v_mfma_f32_32x32x16_bf16.  Parameters, gradients, optimizer state, stored activations and all
 * elementwise math stay fp32 either way. */
int cmdgen_train_set_precision(cmdgen_handle* h, int32_t bf16_gemm);

/* Sum of squares of a device vector -> host float (the global gradient norm of utils.get_grad_norm,
 * utils.py:39-61, is its square root).  Synchronises the stream. */
int cmdgen_grad_sqnorm(cmdgen_handle* h, const float* grad, int64_t n, float* out_host, cmdgen_stream stream);

/* One torch.optim.AdamW(amsgrad=True) update (lightning_modules.py:141-143) of the flat buffer, with the norm
 * clipping coefficient of clip_grad_norm_ folded in (pass 1.0 for none; lightning_modules.py:543-568 computes
 * it on the host).  `step` counts from 1.  All pointers dev [n]. */
int cmdgen_adamw_step(cmdgen_handle* h, float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                      float* max_exp_avg_sq, int64_t n, int64_t step, float lr, float beta1, float beta2,
                      float eps, float weight_decay, float clip_coef, cmdgen_stream stream);

/* Gradient norm, clipping and the AdamW update in one queue-up (lightning_modules.py:543-568 + :141-143): the norm of
 * `grad` is reduced on the device, the update applies clip_grad_norm_'s coefficient min(1, max_grad_norm / (norm + 1e-6))
 * formed on the device (max_grad_norm <= 0: no clipping), and the norm comes back in *grad_norm_host for the caller's
 * queue of recent norms - the host round trip between norm and update of cmdgen_grad_sqnorm + cmdgen_adamw_step is gone.
 * Synchronises the stream - unless grad_norm_host is NULL: then the norm is copied to pinned host memory behind the update
 * and cmdgen_last_grad_norm collects it later (it is only needed before the NEXT step's bound is formed), so the host can
 * queue the next step's noising and graph build while this step's backward pass is still running. */
int cmdgen_adamw_step_clipped(cmdgen_handle* h, float* theta, const float* grad, float* exp_avg, float* exp_avg_sq,
                              float* max_exp_avg_sq, int64_t n, int64_t step, float lr, float beta1, float beta2,
                              float eps, float weight_decay, float max_grad_norm, float* grad_norm_host,
                              cmdgen_stream stream);
/* The norm of the last cmdgen_adamw_step_clipped called with grad_norm_host = NULL (waits for that update only). */
int cmdgen_last_grad_norm(cmdgen_handle* h, float* grad_norm_host);

/* After a training forward on the half matrix engine, cmdgen_adamw_step_clipped skips the update - its norm comes back
 * non-finite - when that forward took a NaN reset or counted rows below the engine's range (cmdgen_counters.half_low_range).
 * This call writes that range event of the last cmdgen_train_forward to dev out[0], stream-ordered: 0 for none, +1 for a NaN
 * reset, +4096 for low-range rows (0 after a forward off the half engine); the next cmdgen_adamw_step_clipped's guard then
 * reads out[0] instead of this process's own event.  A data-parallel caller sums the slot over its ranks (with the gradient
 * all-reduce) before the update, so that every rank skips the same step.  cmdgen_query "train_range_event" returns the
 * value the guard read, once cmdgen_last_grad_norm (or a waiting update) has brought the norm back. */
int cmdgen_train_range_event(cmdgen_handle* h, float* out, cmdgen_stream stream);

/* C[M,N] (+)= op(A) op(B) (+ bias) through the training path's exact-fp32 MFMA GEMM (test aid):
 * ta: A stored [K][M]; tb: B stored [N][K] (nn.Linear weight); accumulate bit 0: C += ..., bit 1: bf16 operands. */
int cmdgen_debug_sgemm(cmdgen_handle* h, int32_t ta, int32_t tb, int32_t M, int32_t N, int32_t K, const float* A,
                       int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc, const float* bias,
                       int32_t accumulate, int32_t split_k, cmdgen_stream stream);

/* Optional: supply the per-step scalars of sample_p_zs_given_zt computed by the host
 * (e.g. with the same torch fp32 ops as the reference, bit for bit) instead of the
 * library's own libm evaluation.  coef_host is [K+1][4]:
 *   rows 0..K-1 (s = K-1 .. 0): alpha_ts, sigma2_ts/alpha_ts/sigma_t, sigma_ts*sigma_s/sigma_t, t
 *   row  K     (final decode) : sigma_0, alpha_0, exp(gamma_0/2), 0
 * (conditional_model.py:345-366, :108-131; en_diffusion.py:79-103).  Used by the next
 * cmdgen_sample_chain whose `timesteps` equals K. */
int cmdgen_set_step_table(cmdgen_handle* h, int32_t K, const float* coef_host);

/* Optional, beside the step table: sigma_t and alpha_t of every posterior op (rows s = K-1 .. 0, t = (s+1)/K; [K][2]) for the
 * denoised estimate of cmdgen_restrained_chain, computed by the host with the reference's own fp32 ops.  Used by the next
 * cmdgen_restrained_chain whose `timesteps` equals K; otherwise the library evaluates both from its gamma table. */
int cmdgen_set_guide_table(cmdgen_handle* h, int32_t K, const float* sigma_alpha_host);

/* Deferred, non-syncing versions of the reference's in-loop checks, read back after the
 * chain (synchronises the stream):
 *   max_rel_com_error : max over steps of assert_mean_zero_with_mask's relative error
 *                       (en_diffusion.py:919-924; the reference asserts < 1e-2)
 *   max_cog           : the final CoG drift (conditional_model.py:451-457)
 *   nan_resets        : evaluations whose output was reset by the NaN guard */
int cmdgen_chain_status(cmdgen_handle* h, float* max_rel_com_error, float* max_cog,
                        int64_t* nan_resets, cmdgen_stream stream);

/* ---- measurement ------------------------------------------------------------------ */
int cmdgen_get_counters(cmdgen_handle* h, cmdgen_counters* out, cmdgen_stream stream); /* syncs */
int cmdgen_reset_counters(cmdgen_handle* h, cmdgen_stream stream);
/* Runs ONE evaluation on the current inputs with a hipEvent pair around every launch and
 * returns the per-kernel sums (synchronises). */
int cmdgen_profile_evaluation(cmdgen_handle* h, const float* xh_phar, const float* xh_pocket,
                              const float* t, float* eps_phar, cmdgen_kernel_times* out,
                              cmdgen_stream stream);
/* Y[M,256] (+)= (A0 W0 + A1 W1) / div * SiLU'(pre) through the training step's data-gradient kernel (test aid; A1 / pre may be
 * NULL): W0 / W1 dev [256][256] row-major nn.Linear weights (dX = dY W; when both are given they must lie in ONE device
 * allocation), packed as the step packs them.  pieces: 3 = fp32-accurate split products, 1 = bf16 operands; tile_rows: 0 =
 * the launcher's choice, 32 / 64 = forced.  Synchronises the stream. */
int cmdgen_debug_dgrad(cmdgen_handle* h, int32_t M, const float* A0, const float* W0, const float* A1, const float* W1,
                       float* Y, int32_t accumulate, float div, const float* pre, int32_t pieces, int32_t tile_rows,
                       cmdgen_stream stream);

/* dW[M,N] += dY^T X (dY dev [K,M], X dev [K,N], both contiguous), db[M] += column sums of dY (db may be NULL), through the
 * training step's weight-gradient launch (test aid).  mode 0 = fp32 instruction, 1 = bf16 operands, 3 = three-piece split
 * where the shape allows, otherwise as 0). */
int cmdgen_debug_wgrad(cmdgen_handle* h, int32_t K, int32_t M, int32_t N, const float* dY, const float* X, float* dW,
                       float* db, int32_t mode, cmdgen_stream stream);

/* Matrix engine of the tile kernels (evaluation, chains, and the fp32 products of the training step: its two forward
 * edge kernels and every [.,256] x [256,256] data gradient; cmdgen_train_set_precision is the separate bf16-OPERAND switch):
 *   1 (default) = split-bf16: every fp32 operand is the exact sum of three bf16 pieces and every fp32 product is six
 *       exact bf16 products accumulated in fp32 on v_mfma_f32_32x32x16_bf16 - fp32-accurate (the dropped terms are
 *       <= 3 * 2^-24 |a||b|, below the fp32 accumulation rounding both engines share) at about twice the delivered
 *       rate of the fp32 matrix instruction; used by tiles of >= 32 rows;
 *   0 = v_mfma_f32_32x32x2_f32 / 16x16x4_f32 everywhere (bitwise an fmaf chain).
 * 16-row node tiles use v_mfma_f32_16x16x32_bf16 the same way (option "node16_split"), 16-row edge / embedding tiles
 * the fp32 instruction.  Changing the mode drops captured step graphs (they are re-captured on the next chain) and
 * re-picks the tile sizes of the current layout. */
int cmdgen_set_gemm_mode(cmdgen_handle* h, int32_t split_bf16);

/* Explicit launch choices of ONE handle (measurement, parity tests, A/B runs).  The library reads no environment variable:
 * everything that used to be a CMDGEN_* switch is a key here.  unset != 0 removes the key (back to the library's own
 * choice; `value` ignored).  Setting an option drops captured step graphs and re-picks the tiles of the current layout.
 *   rows per tile        "node_mt" 16|32|64, "edge_mt" / "coord_mt" 16|32|64|128 (128: kernels_edge128.hip, split engine,
 *                        hidden_nf 256), "embed_mt" 16|32|64
 *   grids                "edge_wgs_per_cu", "coord_wgs_per_cu" (persistent-style edge grids of the <= 64-row kernels),
 *                        "e128_wgs_per_cu" 1|2, "e128_fused" 0..3 (bit 0 / 1: the 128-row message / coordinate kernel issues the next quarter's
 *                        tile build inside its GEMM; default: by the estimated list length - more than one tile per workgroup)
 *   matrix engine        "half_engine" 0|1|2: the split-engine kernels that have a HALF form (two fp16 pieces per operand, three MFMAs per
 *                        fp32 product instead of three bf16 pieces and six; csrc/cmdgen_split.h) use it: 1 (default) when the model has an
 *                        edge cutoff (the radial features are bounded; fp16 ends at 65504), 2 always, 0 never
 *   kernel variants      "edge_fullk" 0|1 (full-K planes for 32-row edge tiles), "node64" 0|1|32 (64-row planes node kernel;
 *                        32: its 32-row form), "node16_split" 0|1, "node16w" 0|1 (16-row node tiles of H = 256 on eight waves,
 *                        kernels_node16w.hip; default 1), "write_embed" 0|1 (graph pass 2 + k_embed in one launch),
 *                        "proj_in_coord" 0|1 (the next block's P | Q projections as 32-row x 128-column tiles inside the coordinate launch
 *                        instead of inside k_node16w - kernels_coord_proj.hip; same bits.  It exists only where k_node16w takes the node
 *                        launches and the coordinate list runs on the 32-row full-K tile, conditional model, inv_sublayers 1, hidden_nf 256:
 *                        1 = wherever that holds, 0 = never, unset = the library's rule (the same places).  Training forwards,
 *                        cmdgen_debug_eval_prefix and cmdgen_profile_evaluation always keep the projections in the node launch.)
 *                        "embed_mfma" 0|1 (the full-path 16-row embedding tiles whose rows are all phar rows run encoder layer 2 and the
 *                        embedding on v_mfma_f32_16x16x4_f32, C = bias and k ascending, with every operand requested at kernel start; same
 *                        bits as the scalar tile.  hidden_nf 256, phar_nf 8, joint_nf 32 with the time column, 16-row tiles, never the training
 *                        forward: 1 = wherever that holds, 0 = never, unset = the library's rule: there, from 30 such tiles - 480 phar rows)
 *                        "readout_in_coord" 0|1 (cmdgen_sample_chain runs without k_readout: embedding_out and the decoders of the phar rows as
 *                        tiles of the last block's coordinate launch - kernels_coord_proj.hip -, the velocity and the batch-global NaN flag formed
 *                        by the step kernel that consumes them, X0 / ACC handed from the step kernel to pass 2 of the radius graph; same bits.
 *                        It exists only where the coordinate list runs on the 32-row full-K tile, conditional model, inv_sublayers 1, hidden_nf
 *                        256, joint_nf + 1 <= 40, samples of at most 128 nodes: 1 = wherever that holds, 0 = never, unset = the library's rule
 *                        (the same places).  Every other chain and entry point keeps k_readout.)
 *   dead work            "dead_skip" 0|1|2 (2, default: every block skips tiles beyond L - l hops of a moving node; 1: the
 *                        last block only; 0: off)
 *   chain                "graph_steps" (denoising steps per captured graph, default 8)
 *   training step        "wgrad_split" -1|0|1 (-1: three-piece weight gradients wherever the handle runs the split engine), "wgrad_tile" 0|64, "wgrad_split_wgs128", "wgrad_split_wgs64", "wgrad_wgs",
 *                        "dgrad_mt" 0|32|64, "dgrad_tail" 0|1   (see TrainTune in csrc/cmdgen_train_plan.h);
 *                        "wgrad_stream" 0|1|2 (weight / bias gradients and partial-sum reductions on the handle's second stream beside the chain
 *                        of data gradients; 2: at the lowest stream priority; default 1), "train_half" 0|1|2 (the training forward's tile kernels on
 *                        the half engine, packs and scales re-made on the device every step; 2: the two edge kernels only; default 1 where
 *                        "half_engine" resolves on),
 *                        "wgrad_silu" 0..3 (bit 0 / 1: SiLU(pre1) / SiLU(pre6) are not stored by the forward but formed by the second layer's
 *                        weight gradient; default 3 with bf16 operands, 0 for fp32 results), "wgrad_k128" (rows x 128-tiles of a launch from which a
 *                        three-piece weight gradient uses 128 x 128 tiles; default 131072), "train_node16" 0|1 (16-row node tiles in the training
 *                        forward at every batch size; default 1)
 *   (round 6: the options whose A/B lost - "e128_pp", "dgrad_half", "small_wgrads" - left the build: profiles/r06_removed_experiments.patch)
 * cmdgen_get_option: *value = the stored value, *is_set = 0 when the key is not set (either pointer may be NULL).
 * Unknown keys: CMDGEN_EINVAL. */
int cmdgen_set_option(cmdgen_handle* h, const char* key, int64_t value, int32_t unset);
int cmdgen_get_option(cmdgen_handle* h, const char* key, int64_t* value, int32_t* is_set);

/* Diagnostic builds only (kernels compiled with -DCMDGEN_STAMPS): 64 summed in-kernel cycle stamps of k_edge_msg
 * ([wave][phase], wave lifetimes, wave count); all zero in production builds.  Synchronises the device. */
int cmdgen_debug_stamps(cmdgen_handle* h, uint64_t* out64, int32_t reset);

/* Launch configuration in force for the current layout (measurement aid): key = "node_mt" | "edge_mt" | "coord_mt"
 * (rows per tile of the three MFMA kernels), "edge_grid" | "coord_grid" (workgroups of the persistent-style edge
 * kernels), "gemm_split" (the mode above), "node16_split", "node16w", "node64", "edge_fullk", "dead_skip", "proj_in_coord", "embed_mfma", "readout_in_coord" (as resolved from the
 * options and the layout), "chain_graphs" (captured step graphs the handle holds), "half_engine" (the engine option as resolved: 1 = kernels with a half form use it), "msg_mfmas_per_product" |
 * "node_mfmas_per_product" | "coord_mfmas_per_product" (1: the fp32 matrix instruction, 6: three bf16 pieces per operand, 3: two fp16 pieces - the
 * engine the three tile kernels of the current layout run on), "train_edges" | "train_coord_edges" (edges of the last cmdgen_train_forward). */
int cmdgen_query(cmdgen_handle* h, const char* key, int64_t* value);

/* Steady-state timing of one network evaluation (bench.py's trained-geometry micro-benchmark): `graph_len`
 * evaluations of the given inputs are captured into a hipGraph, replayed `replays` times after one warm-up replay
 * and timed with HIP events on the launch stream.  *mean_ms = time per evaluation.  Counters advance as usual. */
int cmdgen_time_evaluation(cmdgen_handle* h, const float* xh_phar, const float* xh_pocket, const float* t,
                           float* eps_phar, int32_t graph_len, int32_t replays, float* mean_ms, cmdgen_stream stream);

/* Replays the edge-message kernel of block `layer` `reps` times on the state left by the
 * last evaluation and returns the mean launch duration in ms (hipEvents on `stream`). */
int cmdgen_time_edge_kernel(cmdgen_handle* h, int32_t layer, int32_t reps, float* mean_ms,
                            cmdgen_stream stream);

/* Per-launch timing of the three MFMA kernels inside a real chain: while enabled, every eager
 * (use_graph = 0) launch of k_edge_msg / k_node / k_edge_coord is bracketed by a hipEvent pair on
 * the launch stream.  cmdgen_get_kernel_profile synchronises and returns, per kernel class
 * (CMDGEN_K_EDGE_MSG, CMDGEN_K_NODE, CMDGEN_K_EDGE_COORD), the summed duration and the number of
 * launches since the last call; it clears the record. */
#define CMDGEN_K_EDGE_MSG   0
#define CMDGEN_K_NODE       1
#define CMDGEN_K_EDGE_COORD 2
int cmdgen_set_kernel_profiling(cmdgen_handle* h, int32_t on);
int cmdgen_get_kernel_profile(cmdgen_handle* h, float total_ms[3], int64_t launches[3], cmdgen_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* CMDGEN_HIP_H */
