// cmdgen_host.h - host-side state shared by cmdgen_api.hip and cmdgen_train.hip
#pragma once
#include "cmdgen_dev.h"
#include "../../include/cmdgen_hip.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

extern std::string g_create_error;
struct TrainState;               // cmdgen_train.hip
void cmdgen_train_free(TrainState*);


struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
};

// A slot's table block as its entry lays it out (cmdgen_api.hip): the posterior (scoring: level) rows | the edit tables | the group tables |
// the guidance tail | the sets' tail (the diverse kinds; the restrained diverse kind has both) - whatever must prepare the slot again when it changes.  Each appender records where its section begins, so nothing
// derives an offset a second time.
struct TableBlock {
    std::vector<float> f;                  // the upload
    size_t edit = 0, groups = 0, guide = 0; // float offset of the edit tables (coef2 | iop), the group tables, the guidance tail; 0: the block has none
    int guide_rows = 0;                    // guide rows of the tail
    int owners = 0;                        // owners of the tail's restraints (the layout's samples, or the groups): its CSR offsets are [owners + 1]
    int G = 0;                             // groups of the group tables; nothing reads it back (a call's counts come from its GroupPlan) - it is part of the slot's key only
    size_t sets = 0;                       // float offset of the diverse chain's tail (guide rows | scalars | set tables, append_sets); 0: the block has none
    bool same(const TableBlock& o) const {
        return edit == o.edit && groups == o.groups && guide == o.guide && guide_rows == o.guide_rows && owners == o.owners && G == o.G && sets == o.sets &&
               f.size() == o.f.size() && memcmp(f.data(), o.f.data(), f.size() * sizeof(float)) == 0;
    }
};

// Host state of one kind of denoising chain (cmdgen_api.hip): its buffers for the current layout, the plan tables they were
// prepared for, and its captured steps.  Each kind has a slot of its own, so plain and inpainting chains alternate on a
// handle without re-preparing or re-capturing.
enum ChainKind { CHAIN_PLAIN, CHAIN_JOINT, CHAIN_INPAINT, CHAIN_SCORE, CHAIN_MULTI, CHAIN_MULTI_EDIT, CHAIN_MULTI_SCORE, CHAIN_RESTRAINED, CHAIN_RESTRAINED_EDIT, CHAIN_MULTI_RESTRAINED, CHAIN_MULTI_RESTRAINED_EDIT, CHAIN_DIVERSE, CHAIN_DIVERSE_RESTRAINED, CHAIN_KINDS };
struct ChainSlot {
    std::vector<void*> allocs;
    TableBlock tables;                     // the uploaded table block with its offsets, compared to decide a re-prepare
    int n_steps = -1;                      // denoising steps of the prepared plan (-1: nothing prepared)
    unsigned int* check = nullptr;         // [n_steps+3][2] (cmdgen_chain_status)
    ChainState* state = nullptr;
    unsigned int* cog = nullptr;           // CoG drift of the final sample
    float* pk[7] = {};                     // PocketCache storage (c, P0, Q0, dh, dP, dQ) and the time pair (0, 1) that builds it
    hipGraphExec_t graph = nullptr;        // G captured steps, valid for the key below
    const void* key[6] = {};               // what the captured steps bake in: five caller pointers and the stream
    unsigned long long seed = 0;
    int graph_steps = 0;
    // the kernel arguments the buffers above back: filled by the kind's ChainAlloc, copied and completed per call by its entry
    ChainBuf buf{};                        // every conditional kind: z, the pocket, the posterior (scoring: level) rows, checks and state
    InpaintBuf inp{};                      // edit kinds: the op tables, the known rows and marks (multi-pocket: once per group), the offset per sample
    GroupTab groups{};                     // multi-pocket kinds: the group tables in the slot's table block (a changed grouping prepares the slot again)
    RestrainBuf restr{};                   // restrained kinds (the restrained diverse kind among them): the guidance tables in the slot's table block (a changed restraint prepares the slot again)
    float* guide_d = nullptr;              // restrained multi-pocket kinds: the displacement of every group's rows [Nu][3], written by the guide launch for the step launch
    DiverseBuf div{};                      // diverse kinds: the guide rows, scalars and set tables in the slot's table block (a changed partition or scalar prepares the slot again), y, gd, po
    ScoreBuf score{};                      // scoring kinds: the clean rows the levels noise
    JointBuf joint{};                      // joint kind: its z, scratch and plan rows ...
    float* eps_pocket = nullptr;           // ... and the pocket output [Np][3+R] of its evaluations
};

struct cmdgen_handle {
    cmdgen_config cfg{};
    int device = 0;
    std::string err;
    Dims dims{};
    // weights
    std::map<std::string, std::vector<float>> staged;
    bool finalized = false;
    std::vector<void*> weight_allocs;
    std::vector<LayerW> layers;
    SmallW small{};
    std::vector<float> gamma;              // host copy of the table [T+1]
    // layout + workspace
    bool have_layout = false;
    std::vector<int64_t> cur_nphar, cur_npocket;
    std::vector<void*> layout_allocs;
    Layout lay{};
    Work work{};
    int64_t ecap = 0, eccap = 0;
    int64_t cap_B = 0, cap_Nl = 0, cap_Np = 0, cap_N = 0, cap_e = 0, cap_ec = 0;   // allocated capacities of the workspaces
    int n_cus = 256;
    LaunchPlan plan;                       // the sampler's launch plan for the current layout, options, engine and weights (replan)
    bool gemm_split = true;                // tiles of >= 32 rows multiply on the bf16 matrix pipe (cmdgen_set_gemm_mode)
    int64_t* d_gid = nullptr;
    int* idx_blk[2] = {nullptr, nullptr};  // two copies of the index block: a new layout is written to the one the previous layout's kernels do not read
    int* idx_stage[2] = {nullptr, nullptr}; // pinned staging of the same size (cmdgen_set_layout_on_stream)
    hipEvent_t idx_ev[2] = {nullptr, nullptr};
    int idx_cur = 0;
    int64_t idx_ints = 0;
    // chains
    ChainSlot chains[CHAIN_KINDS];
    ChainKind last_chain = CHAIN_PLAIN;    // the kind cmdgen_chain_status reports on
    std::vector<float> user_coef;          // optional host-supplied step table
    int user_coef_K = -1;
    std::vector<float> user_guide;         // optional host-supplied guide table [K][2] (cmdgen_set_guide_table)
    int user_guide_K = -1;
    hipStream_t own_stream = nullptr;      // used when the caller's stream is the legacy default stream (not capturable)
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    TrainState* train = nullptr;           // training workspace (cmdgen_train.hip)
    float* h_norm = nullptr; hipEvent_t norm_ev = nullptr; bool norm_pending = false;   // deferred gradient-norm readback (pinned host float)
    int train_E = 0, train_Ec = 0;         // message / coordinate edges of the last cmdgen_train_forward (cmdgen_query)
    int64_t eval_gen = 0;                  // bumped by every call that rewrites the evaluation workspace (edge lists, flags) or the layout:
                                           // cmdgen_train_backward_inputs refuses activations whose graph is no longer the handle's
    int64_t train_gen = -1;                // eval_gen of the last cmdgen_train_forward
    int train_fwd_half = 0;                // the last cmdgen_train_forward's tile kernels ran on the half engine (cmdgen_query "train_half_ran")
    bool train_bf16 = false;               // GEMM operand precision of the training step (cmdgen_train_set_precision)
    bool agg_dirty = false;                // cmdgen_debug_eval_prefix left segment sums in work.agg
    hipStream_t last_stream = nullptr;     // stream most recently handed to this handle (ordering contract of cmdgen_set_layout)
    std::map<std::string, int64_t> opts;   // cmdgen_set_option: explicit launch choices of this handle (absent key = the library's own choice)
    TrainTune tune{};                      // the training step's part of them
    bool kernel_profiling = false;
    std::vector<hipEvent_t> prof_events[3];
};

inline int fail(cmdgen_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}
#define HIPCHK(h, call) do { hipError_t _e = (call); if (_e != hipSuccess) \
    return fail(h, CMDGEN_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); } while (0)

inline int dev_alloc(cmdgen_handle* h, std::vector<void*>& pool, void** out, size_t bytes, bool zero) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(out, bytes);
    if (e != hipSuccess) return fail(h, CMDGEN_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    pool.push_back(*out);
    if (zero) { e = hipMemset(*out, 0, bytes); if (e != hipSuccess) return fail(h, CMDGEN_EHIP, "hipMemset failed"); }
    return 0;
}
inline void free_pool(std::vector<void*>& pool) { for (void* p : pool) hipFree(p); pool.clear(); }


int check_ready(cmdgen_handle* h);
int begin_work(cmdgen_handle* h, hipStream_t s);   // check_ready + device + workspace invariants; remembers the stream
PlanInput plan_input(const cmdgen_handle* h);      // the sampler's planner input: dims, layout, options, engine, the packs the weights have
void replan(cmdgen_handle* h);                     // h->plan again: after a new layout, option, engine or set of weights
EvalLaunch make_launch(cmdgen_handle* h);
inline int64_t opt_of(const cmdgen_handle* h, const char* key, int64_t dflt) { auto it = h->opts.find(key); return it == h->opts.end() ? dflt : it->second; }
inline bool opt_set(const cmdgen_handle* h, const char* key) { return h->opts.find(key) != h->opts.end(); }
