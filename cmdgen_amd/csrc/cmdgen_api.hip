// cmdgen_api.hip - the C ABI of libcmdgen_hip.so (include/cmdgen_hip.h): handle, weight
// packing, workspaces, the launch sequence of one evaluation and the denoising loop
// (eager or replayed as a hipGraph).
#include "cmdgen_host.h"
#include "cmdgen_launch.h"
#include "cmdgen_wlayout.h"

std::string g_create_error;

extern "C" const char* cmdgen_version(void) { return "cmdgen_hip 0.1 (gfx950)"; }

extern "C" const char* cmdgen_last_error(const cmdgen_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

extern "C" int cmdgen_create(const cmdgen_config* cfg, int device, cmdgen_handle** out) {
    if (!cfg || !out) return fail(nullptr, CMDGEN_EINVAL, "null argument");
    const int H = cfg->hidden_nf;
    if (!(H == 64 || H == 128 || H == 256 || H == 512))
        return fail(nullptr, CMDGEN_EINVAL, "hidden_nf=%d unsupported: the gfx950 kernels tile 64 columns per wave and are built for 64, 128, 256 and 512", H);
    if (cfg->inv_sublayers < 1 || cfg->inv_sublayers > 8) return fail(nullptr, CMDGEN_EINVAL, "inv_sublayers=%d out of range [1, 8]", cfg->inv_sublayers);
    if (cfg->n_layers < 1 || cfg->n_layers > CMDGEN_MAX_LAYERS) return fail(nullptr, CMDGEN_EINVAL, "n_layers out of range");
    if (cfg->phar_nf < 1 || 2 * cfg->phar_nf > CMDGEN_MAX_SMALL || cfg->residue_nf < 1 ||
        2 * cfg->residue_nf > CMDGEN_MAX_SMALL || cfg->joint_nf < 1 || cfg->joint_nf + 1 > CMDGEN_MAX_SMALL)
        return fail(nullptr, CMDGEN_EINVAL, "feature sizes exceed the small-MLP bound %d", CMDGEN_MAX_SMALL);
    if (cfg->timesteps < 1) return fail(nullptr, CMDGEN_EINVAL, "timesteps < 1");
    if (cfg->update_pocket_coords && cfg->no_com_projection)
        return fail(nullptr, CMDGEN_EINVAL, "update_pocket_coords (joint model) and no_com_projection (SimpleConditionalDDPM) are exclusive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(nullptr, CMDGEN_EHIP, "no usable HIP device %d (found %d)", device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, CMDGEN_EHIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, CMDGEN_EINVAL, "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, CMDGEN_EHIP, "hipSetDevice failed");
    cmdgen_handle* h = new cmdgen_handle();
    h->cfg = *cfg; h->device = device;
    Dims& d = h->dims;
    d.P = cfg->phar_nf; d.R = cfg->residue_nf; d.J = cfg->joint_nf; d.H = H; d.L = cfg->n_layers;
    d.condition_time = cfg->condition_time ? 1 : 0; d.dyn = d.J + d.condition_time;
    d.attention = cfg->attention ? 1 : 0; d.use_tanh = cfg->tanh ? 1 : 0; d.no_com = cfg->no_com_projection ? 1 : 0;
    d.joint = cfg->update_pocket_coords ? 1 : 0;
    d.cutoff2 = cfg->edge_cutoff < 0.f ? -1.f : cfg->edge_cutoff * cfg->edge_cutoff;
    d.norm_constant = cfg->norm_constant; d.norm_factor = cfg->normalization_factor; d.coords_range = cfg->coords_range;
    d.S = cfg->inv_sublayers; d.agg_mean = cfg->aggregation_mean ? 1 : 0;
    d.sin = cfg->sin_embedding ? 1 : 0;
    {   // SinusoidsEmbeddingNew.frequencies (egnn_new.py:252): 2 * pi * 4 ** arange(6) / 15 as torch evaluates it in fp32
        const float two_pi = (float)6.283185307179586;
        float p4 = 1.0f;
        for (int k = 0; k < 6; ++k) { d.sin_freq[k] = (two_pi * p4) / 15.0f; p4 *= 4.0f; }
    }
    d.norm_x = cfg->norm_x; d.norm_h = cfg->norm_h; d.bias_h = cfg->bias_h;
    h->n_cus = prop.multiProcessorCount;
    if ((size_t)(8 + d.dyn) * H * sizeof(float) > 64 * 1024) cmdgen_readout_allow_lds((size_t)(8 + d.dyn) * H * sizeof(float));
    h->gemm_split = !d.sin;                           // matrix engine of the tiles of >= 32 rows (cmdgen_set_gemm_mode); sin_embedding: the fp32
                                                      // instruction (the split engine's plane builders carry the two scalar distance features only)
    *out = h;
    return CMDGEN_OK;
}

// every kind's captured steps (they bake in the kernel choice, the layout and the weights)
static void drop_chain_graphs(cmdgen_handle* h) {
    for (ChainSlot& k : h->chains)
        if (k.graph) { hipGraphExecDestroy(k.graph); k.graph = nullptr; }
}

// every kind's buffers: the next chain of each kind prepares its slot again
static void release_chains(cmdgen_handle* h) {
    for (ChainSlot& k : h->chains) { free_pool(k.allocs); k.n_steps = -1; k.tables = TableBlock{}; }
}

extern "C" void cmdgen_destroy(cmdgen_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    drop_chain_graphs(h);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    if (h->ev_in) hipEventDestroy(h->ev_in);
    if (h->ev_out) hipEventDestroy(h->ev_out);
    release_chains(h);
    free_pool(h->weight_allocs); free_pool(h->layout_allocs);
    for (int i = 0; i < 2; ++i) { if (h->idx_stage[i]) hipHostFree(h->idx_stage[i]); if (h->idx_ev[i]) hipEventDestroy(h->idx_ev[i]); }
    if (h->h_norm) hipHostFree(h->h_norm);
    if (h->norm_ev) hipEventDestroy(h->norm_ev);
    cmdgen_train_free(h->train);
    delete h;
}

// ---------------------------------------------------------------------------------
// weights
// ---------------------------------------------------------------------------------
extern "C" int cmdgen_load_weights(cmdgen_handle* h, const char* name, const float* host, size_t n) {
    if (!h || !name || !host) return fail(h, CMDGEN_EINVAL, "null argument");
    h->staged[name].assign(host, host + n);
    h->finalized = false;
    return CMDGEN_OK;
}

static int get_w(cmdgen_handle* h, const std::string& name, size_t n, const std::vector<float>** out) {
    auto it = h->staged.find(name);
    if (it == h->staged.end()) return fail(h, CMDGEN_ESTATE, "missing tensor '%s'", name.c_str());
    if (it->second.size() != n) return fail(h, CMDGEN_EINVAL, "tensor '%s' has %zu values, expected %zu", name.c_str(), it->second.size(), n);
    *out = &it->second;
    return 0;
}

template <class T, class D>
static int upload(cmdgen_handle* h, const std::vector<T>& v, D* dev) {
    void* p; int rc = dev_alloc(h, h->weight_allocs, &p, v.size() * sizeof(T), false);
    if (rc) return rc;
    if (hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return fail(h, CMDGEN_EHIP, "hipMemcpy H2D failed");
    *dev = (D)p;
    return 0;
}

// W[out][in] in one fragment order (cmdgen_wlayout.h): FR = the order's map, PIECES values of type T per weight, made by split(w, piece[])
template <class FR, int PIECES, class T, class SPLIT>
static std::vector<T> pack(const float* W, int out, int in, SPLIT split) {
    const int NT = out / FR::ROWS, KB = in / FR::KBLK;
    std::vector<T> p((size_t)NT * KB * PIECES * 64 * FR::PER);
    for (int nt = 0; nt < NT; ++nt)
        for (int kb = 0; kb < KB; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < FR::PER; ++j) {
                    T piece[PIECES];
                    split(W[(size_t)FR::row(nt, lane) * in + FR::k0(kb, lane) + FR::koff(j)], piece);
                    for (int s = 0; s < PIECES; ++s) p[wfrag_piece(nt * KB + kb, PIECES, s, lane) * FR::PER + j] = piece[s];
                }
    return p;
}

// round-to-nearest-even bf16 of a finite float (weights are finite: cmdgen_load_weights' callers check)
static inline unsigned short bf16_rne(float f) {
    uint32_t u; memcpy(&u, &f, 4);
    return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
static inline float bf16_val(unsigned short b) { const uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }

static int upload_pack(cmdgen_handle* h, const float* W, int out, int in, WPack* wp) {
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)out * in; ++i) mx = std::max(mx, std::fabs(W[i]));
    const int e = whalf_exp(mx);
    const float sc = whalf_pow2(e);
    wp->wh_scale = sc; wp->wh_inv = whalf_pow2(-e);
    auto f32 = [](float w, float* p) { p[0] = w; };
    auto bf16x3 = [](float w, unsigned short* p) {      // w = p0 + p1 + p2 exactly up to 2^-24 |w| (cmdgen_split.h)
        p[0] = bf16_rne(w); const float r1 = w - bf16_val(p[0]);
        p[1] = bf16_rne(r1); p[2] = bf16_rne(r1 - bf16_val(p[1]));
    };
    auto f16x2 = [sc](float w, _Float16* p) { const float v = w * sc; p[0] = (_Float16)v; p[1] = (_Float16)(v - (float)p[0]); };
    int r = upload(h, pack<WFrag<32, 4>, 1, float>(W, out, in, f32), &wp->w32); if (r) return r;
    r = upload(h, pack<WFrag<16, 4>, 1, float>(W, out, in, f32), &wp->w16); if (r) return r;
    r = upload(h, pack<WFrag<32, 8>, 3, unsigned short>(W, out, in, bf16x3), &wp->ws); if (r) return r;
    r = upload(h, pack<WFrag<32, 8>, 2, _Float16>(W, out, in, f16x2), &wp->wh); if (r) return r;
    wp->wh16 = nullptr; wp->ws16 = nullptr;
    if (in % 128 == 0) {        // the 16-row split / half GEMMs walk four k-blocks of 32 per iteration
        r = upload(h, pack<WFrag<16, 8>, 2, _Float16>(W, out, in, f16x2), &wp->wh16); if (r) return r;
        r = upload(h, pack<WFrag<16, 8>, 3, unsigned short>(W, out, in, bf16x3), &wp->ws16); if (r) return r;
    }
    return 0;
}

extern "C" int cmdgen_finalize_weights(cmdgen_handle* h) {
    if (!h) return CMDGEN_EINVAL;
    hipSetDevice(h->device);
    drop_chain_graphs(h);
    free_pool(h->weight_allocs);
    h->layers.clear(); h->finalized = false;   // a failure below leaves no layer, no pack in the plan and nothing that launches
    if (h->have_layout) replan(h);
    std::vector<LayerW> layers;
    const Dims& d = h->dims;
    const int H = d.H, T = h->cfg.timesteps;
    const std::vector<float>* v; int rc;
#define GET(name, n) do { rc = get_w(h, name, (size_t)(n), &v); if (rc) return rc; } while (0)
#define UP(dst) do { rc = upload(h, *v, &(dst)); if (rc) return rc; } while (0)
    GET("gamma.gamma", T + 1); h->gamma = *v;
    const std::string dy = "dynamics.";
    SmallW& s = h->small;
    GET(dy + "phar_encoder.0.weight", 2 * d.P * d.P); UP(s.pe0_w); GET(dy + "phar_encoder.0.bias", 2 * d.P); UP(s.pe0_b);
    GET(dy + "phar_encoder.2.weight", d.J * 2 * d.P); UP(s.pe2_w); GET(dy + "phar_encoder.2.bias", d.J); UP(s.pe2_b);
    GET(dy + "phar_decoder.0.weight", 2 * d.P * d.J); UP(s.pd0_w); GET(dy + "phar_decoder.0.bias", 2 * d.P); UP(s.pd0_b);
    GET(dy + "phar_decoder.2.weight", d.P * 2 * d.P); UP(s.pd2_w); GET(dy + "phar_decoder.2.bias", d.P); UP(s.pd2_b);
    GET(dy + "residue_encoder.0.weight", 2 * d.R * d.R); UP(s.re0_w); GET(dy + "residue_encoder.0.bias", 2 * d.R); UP(s.re0_b);
    GET(dy + "residue_encoder.2.weight", d.J * 2 * d.R); UP(s.re2_w); GET(dy + "residue_encoder.2.bias", d.J); UP(s.re2_b);
    GET(dy + "residue_decoder.0.weight", 2 * d.R * d.J); UP(s.rd0_w); GET(dy + "residue_decoder.0.bias", 2 * d.R); UP(s.rd0_b);
    GET(dy + "residue_decoder.2.weight", d.R * 2 * d.R); UP(s.rd2_w); GET(dy + "residue_decoder.2.bias", d.R); UP(s.rd2_b);
    {   // the encoders' tensors once more, contiguous, in the order k_embed lays them out in LDS
        std::vector<float> pack;
        for (const char* nm : {"phar_encoder.0.weight", "phar_encoder.0.bias", "phar_encoder.2.weight", "phar_encoder.2.bias",
                               "residue_encoder.0.weight", "residue_encoder.0.bias", "residue_encoder.2.weight", "residue_encoder.2.bias"}) {
            auto it = h->staged.find(dy + nm);
            if (it == h->staged.end()) return fail(h, CMDGEN_ESTATE, "missing tensor '%s%s'", dy.c_str(), nm);
            pack.insert(pack.end(), it->second.begin(), it->second.end());
        }
        rc = upload(h, pack, &s.enc_pack); if (rc) return rc;
    }
    {   // embedding [H][dyn] -> transposed [dyn][H]
        GET(dy + "egnn.embedding.weight", H * d.dyn);
        std::vector<float> t((size_t)H * d.dyn);
        for (int c = 0; c < H; ++c) for (int k = 0; k < d.dyn; ++k) t[(size_t)k * H + c] = (*v)[(size_t)c * d.dyn + k];
        rc = upload(h, t, &s.emb_wT); if (rc) return rc;
        s.emf_pack = nullptr;
        if (d.P == EMF_P && d.J == EMF_J && d.dyn == EMF_J + 1) {
            // B operands of the full-path embedding tile's two MFMA products (embed_body, option embed_mfma), v_mfma_f32_16x16x4_f32 with k ASCENDING: step s
            // of n-tile nt pairs lane l with W[16 nt + l % 16][4 s + l / 16] (WFrag<16, 4> pairs step j with k = 16 kb + 4 g + j, a re-association of the dot
            // product; here the chain must be the scalar form's).  A lane's steps lie behind one another: encoder layer 2, 2 n-tiles x 4 steps, then the
            // embedding, 16 n-tiles x EMF_KE steps (k >= dyn: zero) in EMF_KE_LD floats - 16-byte loads.
            const std::vector<float>* we = v;                       // (both sizes checked by GET)
            GET(dy + "phar_encoder.2.weight", d.J * 2 * d.P);
            const std::vector<float>* w2 = v;
            std::vector<float> pack((size_t)EMF_J * 2 * EMF_P + (size_t)(H / 16) * 64 * EMF_KE_LD, 0.f);
            for (int nt = 0; nt < EMF_J / 16; ++nt) for (int lane = 0; lane < 64; ++lane) for (int st = 0; st < 2 * EMF_P / 4; ++st)
                pack[(size_t)(nt * 64 + lane) * (2 * EMF_P / 4) + st] = (*w2)[(size_t)(16 * nt + lane % 16) * 2 * EMF_P + 4 * st + lane / 16];
            float* pe = pack.data() + EMF_J * 2 * EMF_P;
            for (int nt = 0; nt < H / 16; ++nt) for (int lane = 0; lane < 64; ++lane) for (int st = 0; st < EMF_KE; ++st) {
                const int k = 4 * st + lane / 16;
                pe[(size_t)(nt * 64 + lane) * EMF_KE_LD + st] = k < d.dyn ? (*we)[(size_t)(16 * nt + lane % 16) * d.dyn + k] : 0.f;
            }
            rc = upload(h, pack, &s.emf_pack); if (rc) return rc;
        }
        GET(dy + "egnn.embedding.bias", H); UP(s.emb_b);
    }
    {   // embedding_out [dyn][H] -> transposed [H][dyn]
        GET(dy + "egnn.embedding_out.weight", d.dyn * H);
        std::vector<float> t((size_t)H * d.dyn);
        for (int j = 0; j < d.dyn; ++j) for (int k = 0; k < H; ++k) t[(size_t)k * d.dyn + j] = (*v)[(size_t)j * H + k];
        rc = upload(h, t, &s.embo_wT); if (rc) return rc;
        GET(dy + "egnn.embedding_out.bias", d.dyn); UP(s.embo_b);
    }
    const int nfeat = d.sin ? 24 : 2;            // edge features behind [h_row | h_col]: radial + d0, or 12 + 12 sinusoids (egnn_new.py:174-176)
    const int ld1 = 2 * H + nfeat;
    // one LayerW per GCL ("unit" b * S + sub, egnn_new.py:127-131); the block's EquivariantUpdate rides with its LAST GCL (the node kernel of
    // that unit projects P_c | Q_c), earlier units of a block carry no coordinate weights
    for (int b = 0; b < d.L; ++b)
    for (int sub = 0; sub < d.S; ++sub) {
        LayerW lw{};
        const std::string g = dy + "egnn.e_block_" + std::to_string(b) + ".gcl_" + std::to_string(sub) + ".";
        const std::string c = dy + "egnn.e_block_" + std::to_string(b) + ".gcl_equiv.";
        auto split_first = [&](const std::string& wname, const std::string& bname, WPack* Wpq,
                               const float** bias, const float** wr, const float** wd, const float** we) -> int {
            const std::vector<float>* w; int r = get_w(h, wname, (size_t)H * ld1, &w); if (r) return r;
            // stack [A ; B] as a [2H][H] matrix: rows 0..H-1 = columns 0..H-1 (h_row), rows H.. = columns H..2H-1 (h_col)
            std::vector<float> AB((size_t)2 * H * H);
            std::vector<float> vr(H), vd(H);
            for (int o = 0; o < H; ++o) {
                for (int k = 0; k < H; ++k) {
                    AB[(size_t)o * H + k] = (*w)[(size_t)o * ld1 + k];
                    AB[(size_t)(H + o) * H + k] = (*w)[(size_t)o * ld1 + H + k];
                }
                vr[o] = (*w)[(size_t)o * ld1 + 2 * H]; vd[o] = (*w)[(size_t)o * ld1 + 2 * H + 1];
            }
            r = upload_pack(h, AB.data(), 2 * H, H, Wpq); if (r) return r;
            r = upload(h, vr, wr); if (r) return r; r = upload(h, vd, wd); if (r) return r;
            *we = nullptr;
            if (d.sin) {                   // the 24 feature columns, transposed [24][H]
                std::vector<float> wt((size_t)24 * H);
                for (int o = 0; o < H; ++o) for (int k = 0; k < 24; ++k) wt[(size_t)k * H + o] = (*w)[(size_t)o * ld1 + 2 * H + k];
                r = upload(h, wt, we); if (r) return r;
            }
            const std::vector<float>* bb; r = get_w(h, bname, H, &bb); if (r) return r;
            return upload(h, *bb, bias);
        };
        auto square = [&](const std::string& wname, int in, WPack* Wp) -> int {
            const std::vector<float>* w; int r = get_w(h, wname, (size_t)H * in, &w); if (r) return r;
            return upload_pack(h, w->data(), H, in, Wp);
        };
        rc = split_first(g + "edge_mlp.0.weight", g + "edge_mlp.0.bias", &lw.Wpq_e, &lw.b1, &lw.wr_e, &lw.wd_e, &lw.we_e); if (rc) return rc;
        rc = square(g + "edge_mlp.2.weight", H, &lw.W2); if (rc) return rc;
        GET(g + "edge_mlp.2.bias", H); UP(lw.b2);
        if (d.attention) {
            GET(g + "att_mlp.0.weight", H); UP(lw.wa);
            GET(g + "att_mlp.0.bias", 1); UP(lw.ba);
        } else { lw.wa = lw.b2; lw.ba = lw.b2; }
        rc = square(g + "node_mlp.0.weight", 2 * H, &lw.W3); if (rc) return rc;
        GET(g + "node_mlp.0.bias", H); UP(lw.b3);
        rc = square(g + "node_mlp.2.weight", H, &lw.W4); if (rc) return rc;
        GET(g + "node_mlp.2.bias", H); UP(lw.b4);
        if (sub == d.S - 1) {
            rc = split_first(c + "coord_mlp.0.weight", c + "coord_mlp.0.bias", &lw.Wpq_c, &lw.b6, &lw.wr_c, &lw.wd_c, &lw.we_c); if (rc) return rc;
            rc = square(c + "coord_mlp.2.weight", H, &lw.W7); if (rc) return rc;
            GET(c + "coord_mlp.2.bias", H); UP(lw.b7);
            GET(c + "coord_mlp.4.weight", H); UP(lw.w5);
        } else {                       // never multiplied (the node kernel skips the projection); valid pointers for the bias prefetches
            lw.Wpq_c = lw.Wpq_e; lw.b6 = lw.b1; lw.wr_c = lw.wr_e; lw.wd_c = lw.wd_e; lw.we_c = lw.we_e; lw.W7 = lw.W2; lw.b7 = lw.b2; lw.w5 = lw.b2;
        }
        layers.push_back(lw);
    }
#undef GET
#undef UP
    h->layers = std::move(layers);
    h->finalized = true;
    h->user_coef_K = -1;                       // a new gamma table invalidates any step table
    h->user_guide_K = -1;                      // ... and any guide table
    release_chains(h);
    if (h->have_layout) replan(h);             // the packs exist now
    return CMDGEN_OK;
}

// ---------------------------------------------------------------------------------
// layout
// ---------------------------------------------------------------------------------
// dynamic LDS of k_edge_count / k_edge_write: float4 position + two ints per node (kernels_egnn.hip)
static inline size_t edge_lds_bytes(int max_n) { return (size_t)max_n * (sizeof(float4) + 3 * sizeof(int)); }
static const size_t kEdgeLdsMax = 156 * 1024;      // 160 KiB per CU minus k_edge_write's small static arrays

// The planner's input for the sampler (cmdgen_plan.h holds every rule).
PlanInput plan_input(const cmdgen_handle* h) {
    PlanInput in;
    const Dims& d = h->dims;
    in.H = d.H; in.L = d.L; in.S = d.S; in.dyn = d.dyn; in.joint = d.joint != 0; in.sin = d.sin != 0; in.cutoff = d.cutoff2 >= 0.f;
    in.n_cus = h->n_cus; in.gemm_split = h->gemm_split;
    in.B = (int)h->cur_nphar.size(); in.nph = h->cur_nphar.data(); in.npk = h->cur_npocket.data();
    in.N = h->lay.N; in.Nl = h->lay.Nl; in.max_n = h->lay.max_n;
    in.opts = &h->opts;
    if (!h->layers.empty()) {           // upload_pack's rule (the [2H][H] first-layer stacks and the square layers take H inputs, node_mlp.0 takes 2H)
        in.W2 = in.W7 = in.Wpq_e = PlanPacks::of_uploaded(d.H); in.W3 = PlanPacks::of_uploaded(2 * d.H);
        in.embed_pack = h->small.emf_pack != nullptr;
    }
    return in;
}
void replan(cmdgen_handle* h) { h->plan = make_plan(plan_input(h)); }

static int set_layout_impl(cmdgen_handle* h, int64_t batch, const int64_t* nph, const int64_t* npk, bool on_stream, hipStream_t stream);
extern "C" int cmdgen_set_layout(cmdgen_handle* h, int64_t batch, const int64_t* nph, const int64_t* npk) {
    return set_layout_impl(h, batch, nph, npk, false, nullptr);
}
extern "C" int cmdgen_set_layout_on_stream(cmdgen_handle* h, int64_t batch, const int64_t* nph, const int64_t* npk, cmdgen_stream stream) {
    return set_layout_impl(h, batch, nph, npk, true, (hipStream_t)stream);
}
static int set_layout_impl(cmdgen_handle* h, int64_t batch, const int64_t* nph, const int64_t* npk, bool on_stream, hipStream_t stream) {
    if (!h || batch < 1 || !nph || !npk) return fail(h, CMDGEN_EINVAL, "bad layout arguments");
    if (h->have_layout && (int64_t)h->cur_nphar.size() == batch &&
        memcmp(h->cur_nphar.data(), nph, batch * sizeof(int64_t)) == 0 &&
        memcmp(h->cur_npocket.data(), npk, batch * sizeof(int64_t)) == 0)
        return CMDGEN_OK;
    ++h->eval_gen;
    hipSetDevice(h->device);
    const Dims& d = h->dims;
    const int B = (int)batch;
    std::vector<int> vph(B), vpk(B), bph(B), bpk(B);
    int64_t Nl = 0, Np = 0, ecap = 0, eccap = 0; int max_n = 0;
    for (int b = 0; b < B; ++b) {
        if (nph[b] < 0 || npk[b] < 0) return fail(h, CMDGEN_EINVAL, "negative node count");
        vph[b] = (int)nph[b]; vpk[b] = (int)npk[b]; bph[b] = (int)Nl; bpk[b] = (int)Np;
        Nl += nph[b]; Np += npk[b];
        const int64_t n = nph[b] + npk[b];
        ecap += n * n; eccap += (d.joint ? n : nph[b]) * n;   // dense bound per sample: never overflows
        if (n > max_n) max_n = (int)n;
    }
    const int64_t N = Nl + Np;
    if (N < 1 || ecap > (int64_t)2000000000) return fail(h, CMDGEN_EINVAL, "batch too large for int32 edge indexing (dense bound %lld)", (long long)ecap);
    if (edge_lds_bytes(max_n) > kEdgeLdsMax)
        return fail(h, CMDGEN_EINVAL, "a sample has %d nodes; the per-sample neighbour search keeps positions and offsets in LDS (%d B per node, at most %d nodes)",
                    max_n, 28, (int)(kEdgeLdsMax / 28));
    std::vector<int> ns(N);
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < vph[b]; ++i) ns[bph[b] + i] = b;
        for (int i = 0; i < vpk[b]; ++i) ns[Nl + bpk[b] + i] = b;
    }
    // graphs bake the layout into their kernel arguments; chain buffers are sized by it.  Kernels of the previous
    // layout may still be reading the index arrays rewritten below: wait for the streams this handle has been
    // given (ordering contract in include/cmdgen_hip.h; torch's side streams are non-blocking, so the null-stream
    // copies below are not ordered against them by themselves).
    // (cmdgen_set_layout_on_stream: when the new layout fits the workspaces nothing is waited for - the index arrays go to
    // the OTHER of two device blocks, copied from pinned staging in stream order, so kernels of the previous layout that
    // are still running on `stream` keep reading theirs)
    const bool fits_now = h->cap_B >= B && h->cap_Nl >= Nl && h->cap_Np >= Np && h->cap_N >= N && h->cap_e >= ecap && h->cap_ec >= eccap;
    bool chains_idle = true;
    for (const ChainSlot& k : h->chains) chains_idle = chains_idle && k.allocs.empty() && !k.graph;
    const bool no_wait = on_stream && fits_now && h->have_layout && chains_idle && (h->last_stream == stream);
    if (!no_wait) {
        if (h->own_stream) hipStreamSynchronize(h->own_stream);
        if (h->have_layout) hipStreamSynchronize(h->last_stream);
        if (on_stream) hipStreamSynchronize(stream);
    }
    drop_chain_graphs(h);
    int rc; void* p;
    Layout& L = h->lay; Work& w = h->work;
    // Workspaces are capacity-based: a new batch that fits the current capacities (every training step and every
    // dataset batch has its own ragged layout) only re-uploads the small index arrays - no hipMalloc/hipFree.
    const bool fits = h->cap_B >= B && h->cap_Nl >= Nl && h->cap_Np >= Np && h->cap_N >= N && h->cap_e >= ecap && h->cap_ec >= eccap;
    if (!fits) {
        hipDeviceSynchronize();
        free_pool(h->layout_allocs); release_chains(h);
        cmdgen_train_free(h->train); h->train = nullptr;
        h->have_layout = false;
        auto grow = [](int64_t v) { return v + v / 4 + 64; };
        const int64_t cB = h->cap_B ? grow(B) : B, cNl = h->cap_B ? grow(Nl) : Nl, cNp = h->cap_B ? grow(Np) : Np;
        const int64_t cN = cNl + cNp, ce = h->cap_B ? grow(ecap) : ecap, cec = h->cap_B ? grow(eccap) : eccap;
        const int64_t cNm = d.joint ? cN : cNl;
#define ALLOC(dst, type, count, zero) do { rc = dev_alloc(h, h->layout_allocs, &p, (size_t)(count) * sizeof(type), zero); if (rc) return rc; dst = (type*)p; } while (0)
        // the index arrays live in ONE block, [gid (int64) | num_phar | num_pocket | phar_base | pocket_base | node_sample]: a new
        // layout (every training step has its own) is one host-to-device copy instead of six
        {
            h->idx_ints = 6 * cB + cN;
            for (int i = 0; i < 2; ++i) {
                ALLOC(h->idx_blk[i], int, h->idx_ints, true);
                if (h->idx_stage[i]) hipHostFree(h->idx_stage[i]);
                HIPCHK(h, hipHostMalloc((void**)&h->idx_stage[i], (size_t)h->idx_ints * sizeof(int), hipHostMallocDefault));
                if (!h->idx_ev[i]) HIPCHK(h, hipEventCreateWithFlags(&h->idx_ev[i], hipEventDisableTiming));
            }
            h->idx_cur = 0;
        }
        const size_t H = d.H;
        ALLOC(w.X0, float4, cNm, true); ALLOC(w.XP, float4, cNp, true);
        ALLOC(w.XL, float4, (size_t)d.L * cNm, true); ALLOC(w.ACC, float4, (size_t)d.L * cNm, true);
        ALLOC(w.h, float, cN * H, true); ALLOC(w.P, float, cN * H, true); ALLOC(w.Q, float, cN * H, true);
        ALLOC(w.Pc, float, cN * H, true); ALLOC(w.Qc, float, cN * H, true); ALLOC(w.agg, float, cN * H, true);
        ALLOC(w.adiv, float, cN, true); ALLOC(w.degL, int, cN, true); ALLOC(w.need_qc, int, cN, true); ALLOC(w.pocketE, int, cB, true); ALLOC(w.pocketEph, int, cB, true);
        ALLOC(w.pocketEns, int, cB, true); ALLOC(w.pocketEnsQ, int, cB, true);
        ALLOC(w.erow, int, ce, false); ALLOC(w.ecol, int, ce, false); ALLOC(w.ed0, float, ce, false); ALLOC(w.ehop, int, ce, false);
        ALLOC(w.crow, int, cec, false); ALLOC(w.ccol, int, cec, false); ALLOC(w.cd0, float, cec, false);
        ALLOC(w.totals, int, 4, true); ALLOC(w.counters, unsigned long long, 8, true); ALLOC(w.nan_flag, int, 4, true);
        ALLOC(w.eps_tmp, float, (size_t)cNl * (3 + d.P), true);
        ALLOC(w.dbg, unsigned long long, 64, true);
#undef ALLOC
        h->cap_B = cB; h->cap_Nl = cNl; h->cap_Np = cNp; h->cap_N = cN; h->cap_e = ce; h->cap_ec = cec;
    } else {
        // chain buffers are sized by the exact layout and cheap: rebuilt on the next chain
        release_chains(h);
    }
    if (edge_lds_bytes(max_n) > 64 * 1024) cmdgen_edge_kernels_allow_lds(edge_lds_bytes(max_n));
    L.B = B; L.Nl = (int)Nl; L.Np = (int)Np; L.N = (int)N; L.max_n = max_n;
    L.Nm = d.joint ? (int)N : (int)Nl;
    {
        const int64_t cB = h->cap_B;
        const int cur = (h->idx_cur ^= 1);
        int* blk = h->idx_blk[cur];
        h->d_gid = reinterpret_cast<int64_t*>(blk); L.pocket_gid = h->d_gid;
        L.num_phar = blk + 2 * cB; L.num_pocket = blk + 3 * cB; L.phar_base = blk + 4 * cB; L.pocket_base = blk + 5 * cB;
        L.node_sample = blk + 6 * cB;
        int* stage = h->idx_stage[cur];
        hipEventSynchronize(h->idx_ev[cur]);              // the copy that last used this staging buffer (two layouts ago) is long done
        memset(stage, 0, (size_t)(6 * cB) * sizeof(int));
        int64_t* gid = reinterpret_cast<int64_t*>(stage);
        for (int b = 0; b < B; ++b) {
            gid[b] = b;
            stage[2 * cB + b] = vph[b]; stage[3 * cB + b] = vpk[b]; stage[4 * cB + b] = bph[b]; stage[5 * cB + b] = bpk[b];
        }
        memcpy(stage + 6 * cB, ns.data(), (size_t)N * sizeof(int));
        const size_t bytes = (size_t)(6 * cB + N) * sizeof(int);
        if (no_wait) {
            HIPCHK(h, hipMemcpyAsync(blk, stage, bytes, hipMemcpyHostToDevice, stream));
            HIPCHK(h, hipEventRecord(h->idx_ev[cur], stream));
            HIPCHK(h, hipMemsetAsync(w.agg, 0, (size_t)N * d.H * sizeof(float), stream));
            HIPCHK(h, hipMemsetAsync(w.totals, 0, 4 * sizeof(int), stream));
        } else {
            // (plain hipMemcpy: ordered after all earlier work of the blocking streams that may still read the old arrays)
            HIPCHK(h, hipMemcpy(blk, stage, bytes, hipMemcpyHostToDevice));
            if (fits) {   // reused buffers: restore the invariants a fresh (zeroed) workspace has
                HIPCHK(h, hipMemset(w.agg, 0, (size_t)N * d.H * sizeof(float)));
                HIPCHK(h, hipMemset(w.totals, 0, 4 * sizeof(int)));
            }
        }
    }
    h->ecap = ecap; h->eccap = eccap;
    h->cur_nphar.assign(nph, nph + B); h->cur_npocket.assign(npk, npk + B);
    replan(h);
    h->have_layout = true;
    return CMDGEN_OK;
}

int check_ready(cmdgen_handle* h) {
    if (!h) return CMDGEN_EINVAL;
    if (!h->finalized) return fail(h, CMDGEN_ESTATE, "weights not finalised (cmdgen_finalize_weights)");
    if (!h->have_layout) return fail(h, CMDGEN_ESTATE, "no batch layout (cmdgen_set_layout)");
    return 0;
}

// Entry of every call that queues evaluation work: readiness, device, the stream for cmdgen_set_layout's ordering
// contract, and the workspace invariant "agg is zero between blocks" after a debug prefix run.
int begin_work(cmdgen_handle* h, hipStream_t s) {
    if (!h) return CMDGEN_EINVAL;
    if (!h->have_layout) return fail(h, CMDGEN_ESTATE, "no batch layout (cmdgen_set_layout)");
    hipSetDevice(h->device);
    h->last_stream = s;
    if (h->agg_dirty) {
        HIPCHK(h, hipMemsetAsync(h->work.agg, 0, (size_t)h->lay.N * h->dims.H * sizeof(float), s));
        h->agg_dirty = false;
    }
    return 0;
}

EvalLaunch make_launch(cmdgen_handle* h) {
    EvalLaunch a; a.lay = h->lay; a.w = h->work; a.d = h->dims; a.sw = h->small; a.layers = h->layers.data();
    a.plan = h->plan;
    a.prof_events = nullptr; a.ablate = 0;
    // the graph pass fills the flags only for the kernels that read them
    if (!a.plan.node64 && !a.plan.dead_skip) a.w.need_qc = nullptr;
    a.w.hop_levels = a.plan.dead_skip >= 2 ? h->dims.L : 1;
    if (!a.plan.dead_skip) a.w.ehop = nullptr;
    return a;
}

// ---------------------------------------------------------------------------------
// options
// ---------------------------------------------------------------------------------
static const char* const kOptionKeys[] = {
    "node_mt", "edge_mt", "coord_mt", "embed_mt", "edge_wgs_per_cu", "coord_wgs_per_cu", "e128_wgs_per_cu", "e128_fused", "half_engine", "edge_fullk", "node64", "node16_split", "node16w",
    "proj_in_coord", "embed_mfma", "readout_in_coord", "dead_skip", "write_embed", "graph_steps",
    "wgrad_split", "wgrad_tile", "wgrad_split_wgs128", "wgrad_split_wgs64", "wgrad_wgs", "dgrad_mt", "dgrad_tail", "wgrad_stream", "train_half", "wgrad_silu", "train_node16", "wgrad_k128"};

static void drop_graphs(cmdgen_handle* h) {
    // captured graphs bake the kernel choice in; a replay of the graph destroyed here may still be running
    hipSetDevice(h->device);
    if (h->own_stream) hipStreamSynchronize(h->own_stream);
    if (h->have_layout) hipStreamSynchronize(h->last_stream);
    drop_chain_graphs(h);
}
static void refresh_tune(cmdgen_handle* h) {
    TrainTune t;
    t.wgrad_split = (int)opt_of(h, "wgrad_split", t.wgrad_split); t.wgrad_tile = (int)opt_of(h, "wgrad_tile", t.wgrad_tile);
    t.wgrad_split_wgs128 = (int)opt_of(h, "wgrad_split_wgs128", t.wgrad_split_wgs128); t.wgrad_split_wgs64 = (int)opt_of(h, "wgrad_split_wgs64", t.wgrad_split_wgs64);
    t.wgrad_wgs = (int)opt_of(h, "wgrad_wgs", t.wgrad_wgs); t.dgrad_mt = (int)opt_of(h, "dgrad_mt", t.dgrad_mt); t.dgrad_tail = (int)opt_of(h, "dgrad_tail", t.dgrad_tail);
    t.wgrad_stream = (int)opt_of(h, "wgrad_stream", t.wgrad_stream); t.wgrad_k128 = (int)opt_of(h, "wgrad_k128", t.wgrad_k128);
    h->tune = t;
}

extern "C" int cmdgen_set_option(cmdgen_handle* h, const char* key, int64_t value, int32_t unset) {
    if (!h || !key) return fail(h, CMDGEN_EINVAL, "null argument");
    bool known = false;
    for (const char* k : kOptionKeys) known = known || strcmp(k, key) == 0;
    if (!known) return fail(h, CMDGEN_EINVAL, "unknown option '%s'", key);
    drop_graphs(h);
    if (unset) h->opts.erase(key); else h->opts[key] = value;
    refresh_tune(h);
    if (h->have_layout) replan(h);
    return CMDGEN_OK;
}

extern "C" int cmdgen_get_option(cmdgen_handle* h, const char* key, int64_t* value, int32_t* is_set) {
    if (!h || !key) return fail(h, CMDGEN_EINVAL, "null argument");
    bool known = false;
    for (const char* k : kOptionKeys) known = known || strcmp(k, key) == 0;
    if (!known) return fail(h, CMDGEN_EINVAL, "unknown option '%s'", key);
    if (value) *value = opt_of(h, key, 0);
    if (is_set) *is_set = opt_set(h, key) ? 1 : 0;
    return CMDGEN_OK;
}

// ---------------------------------------------------------------------------------
// one evaluation
// ---------------------------------------------------------------------------------
extern "C" int cmdgen_dynamics_forward(cmdgen_handle* h, const float* xh_phar, const float* xh_pocket,
                                       const float* t, float* eps_phar, float* eps_pocket, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (!xh_phar || !xh_pocket || !t || !eps_phar) return fail(h, CMDGEN_EINVAL, "null device pointer");
    if (h->dims.joint && !eps_pocket) return fail(h, CMDGEN_EINVAL, "joint mode (update_pocket_coords) needs eps_pocket: the pocket velocity is part of the output");
    hipStream_t s = (hipStream_t)stream;
    rc = begin_work(h, s); if (rc) return rc;
    EvalLaunch a = make_launch(h);
    ++h->eval_gen;
    cmdgen_launch_eval(a, xh_phar, xh_pocket, t, nullptr, nullptr, eps_phar, eps_pocket, s, nullptr);
    if (!h->dims.joint) cmdgen_launch_nan_fix(a, eps_phar, s);     // joint: k_vel_com applied the reset already
    HIPCHK(h, hipGetLastError());
    return CMDGEN_OK;
}

extern "C" int cmdgen_debug_eval_prefix(cmdgen_handle* h, const float* xh_phar, const float* xh_pocket, const float* t,
                                        int32_t block, int32_t stage, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (!xh_phar || !xh_pocket || !t) return fail(h, CMDGEN_EINVAL, "null device pointer");
    if (block < 0 || block >= h->dims.L || stage < 1 || stage > 3) return fail(h, CMDGEN_EINVAL, "block in [0, n_layers), stage in 1..3");
    hipStream_t s = (hipStream_t)stream;
    rc = begin_work(h, s); if (rc) return rc;
    EvalLaunch a = make_launch(h);
    ++h->eval_gen;
    a.stop_block = block; a.stop_stage = stage;
    cmdgen_launch_eval(a, xh_phar, xh_pocket, t, nullptr, nullptr, h->work.eps_tmp, nullptr, s, nullptr);
    h->agg_dirty = true;                               // stage 1 leaves the segment sums in agg
    HIPCHK(h, hipGetLastError());
    return CMDGEN_OK;
}

extern "C" int cmdgen_radius_graph(cmdgen_handle* h, const float* x, const int64_t* counts_host, int64_t batch,
                                   int32_t* row_dev, int32_t* col_dev, int64_t cap, int64_t* n_edges, cmdgen_stream stream) {
    if (!h || !x || !counts_host || batch < 1 || !row_dev || !col_dev || !n_edges) return fail(h, CMDGEN_EINVAL, "bad radius-graph arguments");
    hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    const int B = (int)batch;
    std::vector<int> cnt(B), base(B), zeros(B, 0);
    int64_t N = 0, need = 0; int max_n = 0;
    for (int b = 0; b < B; ++b) {
        if (counts_host[b] < 0) return fail(h, CMDGEN_EINVAL, "negative node count");
        cnt[b] = (int)counts_host[b]; base[b] = (int)N; N += counts_host[b]; need += counts_host[b] * counts_host[b];
        if (cnt[b] > max_n) max_n = cnt[b];
    }
    if (N < 1 || need > (int64_t)2000000000) return fail(h, CMDGEN_EINVAL, "bad total node count / dense bound");
    if (cap < need) return fail(h, CMDGEN_EINVAL, "edge capacity %lld below the dense bound %lld", (long long)cap, (long long)need);
    if (edge_lds_bytes(max_n) > kEdgeLdsMax) return fail(h, CMDGEN_EINVAL, "a sample has %d nodes (at most %d)", max_n, (int)(kEdgeLdsMax / 28));
    if (edge_lds_bytes(max_n) > 64 * 1024) cmdgen_edge_kernels_allow_lds(edge_lds_bytes(max_n));
    // every node is presented to the radius-graph kernels as a (non-moving) pocket node of a scratch layout
    std::vector<void*> pool; void* p; int rc = 0;
    Layout L{}; Work w{};
    Dims d = h->dims; d.R = 0; d.joint = 0; d.L = 0;                         // rows of x are [3] wide
#define TMP(dst, type, count) do { if (!rc) { rc = dev_alloc(h, pool, &p, (size_t)(count) * sizeof(type), true); dst = (type*)p; } } while (0)
    int *d_np, *d_zero, *d_base;
    TMP(d_np, int, B); TMP(d_zero, int, B); TMP(d_base, int, B);
    TMP(w.X0, float4, 1); TMP(w.ACC, float4, 1); TMP(w.XP, float4, N); TMP(w.degL, int, N);
    TMP(w.pocketE, int, B); TMP(w.pocketEph, int, B); TMP(w.pocketEns, int, B); TMP(w.pocketEnsQ, int, B);
    TMP(w.ed0, float, need); TMP(w.totals, int, 4); TMP(w.counters, unsigned long long, 8); TMP(w.nan_flag, int, 4);
#undef TMP
    if (rc) { free_pool(pool); return rc; }
    w.erow = row_dev; w.ecol = col_dev;
    hipMemcpy(d_np, cnt.data(), B * sizeof(int), hipMemcpyHostToDevice);
    hipMemcpy(d_base, base.data(), B * sizeof(int), hipMemcpyHostToDevice);
    L.B = B; L.Nl = 0; L.Np = (int)N; L.N = (int)N; L.Nm = 0; L.max_n = max_n;
    L.num_phar = d_zero; L.num_pocket = d_np; L.phar_base = d_zero; L.pocket_base = d_base;
    EvalLaunch a{}; a.lay = L; a.w = w; a.d = d;
    cmdgen_launch_edges(a, x /* no phar rows are read */, x, s);
    hipError_t e = hipStreamSynchronize(s);
    int tot[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpy(tot, w.totals, sizeof tot, hipMemcpyDeviceToHost);
    free_pool(pool);
    if (e != hipSuccess) return fail(h, CMDGEN_EHIP, "radius graph failed: %s", hipGetErrorString(e));
    *n_edges = tot[0];
    return CMDGEN_OK;
}

extern "C" int cmdgen_get_edges(cmdgen_handle* h, int32_t* row, int32_t* col, int64_t cap, int64_t* n_edges, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(h, hipStreamSynchronize(s));
    int tot[2];
    HIPCHK(h, hipMemcpy(tot, h->work.totals, sizeof tot, hipMemcpyDeviceToHost));
    if (n_edges) *n_edges = tot[0];
    const int64_t n = tot[0] < cap ? tot[0] : cap;
    if (n > 0 && row) HIPCHK(h, hipMemcpy(row, h->work.erow, n * sizeof(int), hipMemcpyDeviceToHost));
    if (n > 0 && col) HIPCHK(h, hipMemcpy(col, h->work.ecol, n * sizeof(int), hipMemcpyDeviceToHost));
    return CMDGEN_OK;
}

extern "C" int cmdgen_debug_read(cmdgen_handle* h, const char* what, float* host, size_t n, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    const void* src = nullptr; size_t have = 0;
    const std::string k = what ? what : "";
    const Dims& d = h->dims;
    if (k == "h") { src = h->work.h; have = (size_t)h->lay.N * d.H; }
    else if (k == "agg") { src = h->work.agg; have = (size_t)h->lay.N * d.H; }
    else if (k == "P") { src = h->work.P; have = (size_t)h->lay.N * d.H; }
    else if (k == "Q") { src = h->work.Q; have = (size_t)h->lay.N * d.H; }
    else if (k == "x0") { src = h->work.X0; have = (size_t)h->lay.Nm * 4; }
    else if (k == "xl") { src = h->work.XL; have = (size_t)d.L * h->lay.Nm * 4; }
    else if (k == "acc") { src = h->work.ACC; have = (size_t)d.L * h->lay.Nm * 4; }
    else if (k == "chain_z") {                       // the last conditional chain's z buffer (the multi-pocket chains: every member's copy)
        const ChainSlot& k = h->chains[h->last_chain];   // (the multi-pocket scoring chain: the last level's z; the scoring chain is not served)
        if (h->last_chain == CHAIN_JOINT || h->last_chain == CHAIN_SCORE || !k.buf.z_phar || k.n_steps < 0)
            return fail(h, CMDGEN_ESTATE, "no conditional chain has run on this layout");
        src = k.buf.z_phar; have = (size_t)h->lay.Nl * (3 + d.P);
    }
    else return fail(h, CMDGEN_EINVAL, "unknown debug buffer '%s'", k.c_str());
    if (n > have) n = have;
    HIPCHK(h, hipMemcpy(host, src, n * sizeof(float), hipMemcpyDeviceToHost));
    return CMDGEN_OK;
}

// ---------------------------------------------------------------------------------
// schedule: per-step scalars of sample_p_zs_given_zt, fp32 in the reference's op order
// (en_diffusion.py:79-103, :859-867; conditional_model.py:345-366, :429-433)
// ---------------------------------------------------------------------------------
static inline float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }          // F.softplus, threshold 20
static inline float logsigmoid_f(float x) { return -softplus_f(-x); }
static inline float sigmoid_h(float x) { return 1.0f / (1.0f + expf(-x)); }

static void build_step_table(const std::vector<float>& gamma, int T, int K, std::vector<float>& coef) {
    coef.assign((size_t)(K + 1) * 4, 0.f);
    for (int i = 0; i < K; ++i) {
        const int s = K - 1 - i;
        const float s_arr = (float)s / (float)K, t_arr = (float)(s + 1) / (float)K;
        const float g_s = gamma[(size_t)lrintf(s_arr * (float)T)], g_t = gamma[(size_t)lrintf(t_arr * (float)T)];
        const float sigma2_ts = -expm1f(softplus_f(g_s) - softplus_f(g_t));
        const float alpha_ts = expf(0.5f * (logsigmoid_f(-g_t) - logsigmoid_f(-g_s)));
        const float sigma_ts = sqrtf(sigma2_ts);
        const float sigma_s = sqrtf(sigmoid_h(g_s)), sigma_t = sqrtf(sigmoid_h(g_t));
        coef[i * 4 + 0] = alpha_ts;
        coef[i * 4 + 1] = sigma2_ts / alpha_ts / sigma_t;
        coef[i * 4 + 2] = sigma_ts * sigma_s / sigma_t;
        coef[i * 4 + 3] = t_arr;
    }
    const float g0 = gamma[0];
    coef[K * 4 + 0] = sqrtf(sigmoid_h(g0));          // sigma_0
    coef[K * 4 + 1] = sqrtf(sigmoid_h(-g0));         // alpha_0
    coef[K * 4 + 2] = expf(0.5f * g0);               // SNR(-gamma_0/2)
    coef[K * 4 + 3] = 0.f;                           // t of the final evaluation
}

// Optional: the host supplies the table ([K+1][4], same meaning) computed with its own fp32
// math so that it matches the reference's torch ops bit for bit.
extern "C" int cmdgen_set_step_table(cmdgen_handle* h, int32_t K, const float* coef_host) {
    if (!h || K < 1 || !coef_host) return fail(h, CMDGEN_EINVAL, "bad step table");
    h->user_coef.assign(coef_host, coef_host + (size_t)(K + 1) * 4);
    h->user_coef_K = K;
    return CMDGEN_OK;
}

// the step table of K steps: the caller's when it supplied one for K
static std::vector<float> step_table(const cmdgen_handle* h, int K) {
    std::vector<float> tab;
    if (h->user_coef_K == K) tab = h->user_coef; else build_step_table(h->gamma, h->cfg.timesteps, K, tab);
    return tab;
}

// ---------------------------------------------------------------------------------
// the chains.  The thirteen kinds have three host bodies: sampling_chain (ten kinds: a cube of parts - from the prior or from GIVEN rows,
// one pocket per sample or GROUPS of pockets, unsteered, GUIDEd by restraints, pushed apart within SETS or both), scoring_chain (two kinds: with
// or without groups) and cmdgen_joint_chain.  An extern "C" entry of the first two only packs its arguments (SamplingCall, ScoringCall: a
// part the kind lacks is null) and calls its body; a body branches on the presence of a part, never on the kind.
// A kind's state lives in its slot (h->chains[kind]).  A body reads top to bottom: refusals, the plans of the parts present, the slot's
// table block laid out with the appenders below (TableBlock, cmdgen_host.h: each records where its section begins), Chain::open - whose
// ChainAlloc (alloc_sampling, alloc_scoring, alloc_joint) composes the parts (alloc_chain_buf, alloc_inpaint_part, point_group_tab,
// alloc_restrain_part, alloc_diverse_part, alloc_score_part) at those offsets - the init launches, Chain::start, Chain::steps with the
// corner's step launch, the final launches, Chain::close.
// ---------------------------------------------------------------------------------
static int check_timesteps(cmdgen_handle* h, int K) {
    if (K < 1 || K > h->cfg.timesteps) return fail(h, CMDGEN_EINVAL, "timesteps=%d must be in [1, %d]", K, h->cfg.timesteps);
    return 0;
}
// the conditional chains that neither the joint model nor a no_com_projection handle runs, each with its reason
static const char* const kPocketDiffuses = "its pocket nodes diffuse with the latent";
static const char* const kOwnPocketTerms = "its loss has the pocket's own terms";
static int refuse_joint_no_com(cmdgen_handle* h, const char* what, const char* joint_why, const char* no_com_why = "", int no_com_code = CMDGEN_ESTATE) {
    if (h->dims.joint) return fail(h, CMDGEN_ESTATE, "%s is not supported for the joint model (update_pocket_coords=1): %s", what, joint_why);
    if (h->dims.no_com) return fail(h, no_com_code, "%s is not supported for no_com_projection handles (SimpleConditionalDDPM)%s", what, no_com_why);
    return 0;
}
// injected noise covers the schedule (draws: what the chain calls its rows)
static int check_draws(cmdgen_handle* h, const float* noise, int64_t n_draws, int need, const char* draws = "draws") {
    if (noise && n_draws < need) return fail(h, CMDGEN_EINVAL, "noise holds %lld %s, the schedule needs %lld", (long long)n_draws, draws, (long long)need);
    return 0;
}

// a table block that begins with the posterior (scoring: level) rows `coef`.  They are never empty (a chain has at least one op or level and
// the decode / prior row), so every later section begins at an offset > 0 and 0 can stand for "the block has none" (alloc_sampling)
static TableBlock posterior_rows(std::vector<float> coef) {
    TableBlock t;
    t.f = std::move(coef);
    return t;
}
// ... with a plan's edit tables behind them: coef | coef2 | iop bits
static TableBlock plan_tables(const std::vector<float>& coef, const std::vector<float>& coef2, const std::vector<int>& iop) {
    TableBlock t = posterior_rows(coef);
    t.edit = t.f.size();
    t.f.insert(t.f.end(), coef2.begin(), coef2.end());
    t.f.resize(t.f.size() + iop.size());
    memcpy(t.f.data() + coef.size() + coef2.size(), iop.data(), iop.size() * sizeof(int));
    return t;
}

// the kind's own buffers in its slot's pool, pointed at the uploaded block `dev` by the offsets `t` recorded
typedef int (*ChainAlloc)(cmdgen_handle* h, ChainSlot& k, const TableBlock& t, const float* dev, int n_steps);

// A slot that holds exactly `tables`, bytes and offsets, for the current layout is used as it is, with its captured graph.  Otherwise it
// is prepared again: the tables, the check buffer, the loop state and the CoG slot, then the kind's buffers (alloc).
static int prepare_slot(cmdgen_handle* h, ChainSlot& k, TableBlock& tables, int n_steps, ChainAlloc alloc) {
    if (k.n_steps >= 0 && k.tables.same(tables))
        return 0;
    hipDeviceSynchronize();
    if (k.graph) { hipGraphExecDestroy(k.graph); k.graph = nullptr; }
    free_pool(k.allocs);
    k.n_steps = -1;
    void* p; int rc;
    rc = dev_alloc(h, k.allocs, &p, tables.f.size() * sizeof(float), false); if (rc) return rc;
    HIPCHK(h, hipMemcpy(p, tables.f.data(), tables.f.size() * sizeof(float), hipMemcpyHostToDevice));
    const float* tab = (const float*)p;
    rc = dev_alloc(h, k.allocs, &p, (size_t)(n_steps + 3) * 2 * sizeof(unsigned int), true); if (rc) return rc; k.check = (unsigned int*)p;
    rc = dev_alloc(h, k.allocs, &p, sizeof(ChainState), true); if (rc) return rc; k.state = (ChainState*)p;
    rc = dev_alloc(h, k.allocs, &p, 4 * sizeof(unsigned int), true); if (rc) return rc; k.cog = (unsigned int*)p;
    rc = alloc(h, k, tables, tab, n_steps); if (rc) return rc;
    k.n_steps = n_steps;
    std::swap(k.tables, tables);
    return 0;
}

// storage of the chain-invariant pocket rows of k_embed (PocketCache) and the time pair (t = 0, t = 1) that builds it
static int alloc_pocket_cache(cmdgen_handle* h, ChainSlot& k) {
    const Layout& L = h->lay;
    void* p; int rc;
    for (int i = 0; i < 6; ++i) {            // c, P0, Q0: [Np][H]; dh, dP, dQ: [H]
        rc = dev_alloc(h, k.allocs, &p, (size_t)(i < 3 ? L.Np : 1) * h->dims.H * sizeof(float), true); if (rc) return rc;
        k.pk[i] = (float*)p;
    }
    std::vector<float> t01((size_t)2 * L.B, 0.f);
    for (int b = 0; b < L.B; ++b) t01[L.B + b] = 1.f;
    rc = dev_alloc(h, k.allocs, &p, t01.size() * sizeof(float), false); if (rc) return rc;
    HIPCHK(h, hipMemcpy(p, t01.data(), t01.size() * sizeof(float), hipMemcpyHostToDevice));
    k.pk[6] = (float*)p;
    return 0;
}

// chain-invariant work once per chain: the pocket's features are fixed, so k_embed's output for pocket rows is affine in the
// time feature - two embed-only passes (t = 0, t = 1) give the cache every later evaluation of `a` reads
static void build_pocket_cache(cmdgen_handle* h, const ChainSlot& k, const ChainBuf& c, EvalLaunch& a, hipStream_t s) {
    if (h->lay.Np <= 0) return;
    float* const* pk = k.pk;
    cmdgen_build_pocket_cache(a, c.z_phar, c.xh_pocket, pk[6], pk[0], pk[1], pk[2], pk[3], pk[4], pk[5], s);
    a.pcache = PocketCache{pk[0], pk[1], pk[2], pk[3], pk[4], pk[5]};
}

// the handle's own stream, for work the caller queues on the legacy default stream (which cannot be captured)
static int own_stream(cmdgen_handle* h) {
    if (h->own_stream) return 0;
    HIPCHK(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming));
    return 0;
}

// The start of a chain of `kind` with n_steps denoising steps: the stream it runs on (*s; with use_graph on the legacy default
// stream, the handle's own stream ordered after the caller's pending work), its slot prepared for `tables`, the per-call reset
// (pocket ids of the Philox draws, loop state, check buffer, CoG slot) and the launch description of its evaluations (*a).
static int begin_chain(cmdgen_handle* h, ChainKind kind, TableBlock& tables, int n_steps, ChainAlloc alloc,
                       const int64_t* pocket_ids_host, bool use_graph, hipStream_t caller, hipStream_t* s, EvalLaunch* a) {
    h->last_chain = kind;
    hipSetDevice(h->device);
    int rc;
    *s = caller;
    if (use_graph && caller == nullptr) {
        rc = own_stream(h); if (rc) return rc;
        HIPCHK(h, hipEventRecord(h->ev_in, caller));
        HIPCHK(h, hipStreamWaitEvent(h->own_stream, h->ev_in, 0));
        *s = h->own_stream;
    }
    ChainSlot& k = h->chains[kind];
    rc = prepare_slot(h, k, tables, n_steps, alloc); if (rc) return rc;
    rc = begin_work(h, *s); if (rc) return rc;
    h->last_stream = caller;
    std::vector<int64_t> gid(h->lay.B);                  // global pocket ids for the Philox key
    for (int b = 0; b < h->lay.B; ++b) gid[b] = pocket_ids_host ? pocket_ids_host[b] : b;
    HIPCHK(h, hipMemcpyAsync(h->d_gid, gid.data(), gid.size() * sizeof(int64_t), hipMemcpyHostToDevice, *s));
    HIPCHK(h, hipStreamSynchronize(*s));                 // gid is a stack vector
    const ChainState st0{0, n_steps, 0, 0};
    HIPCHK(h, hipMemcpyAsync(k.state, &st0, sizeof st0, hipMemcpyHostToDevice, *s));
    HIPCHK(h, hipMemsetAsync(k.check, 0, (size_t)(n_steps + 3) * 2 * sizeof(unsigned int), *s));
    HIPCHK(h, hipMemsetAsync(k.cog, 0, 4 * sizeof(unsigned int), *s));
    HIPCHK(h, hipStreamSynchronize(*s));                 // st0 is on the stack
    *a = make_launch(h);
    ++h->eval_gen;
    if (h->kernel_profiling && !use_graph) a->prof_events = h->prof_events;
    return 0;
}

// The n denoising steps of a chain.  The step is identical every iteration (the step index lives on the device), so with
// use_graph G of them (option "graph_steps", default 8: they amortise the per-replay floor of ~10-16 us) are captured once
// and replayed n / G times, and the other n % G run eagerly.  The graph stays valid while its slot keeps its plan
// (prepare_slot) and `key` (the caller's pointers and the stream), the seed and G stay the same.
template <class Step>
static int run_steps(cmdgen_handle* h, ChainSlot& k, const void* const* key, unsigned long long seed, int n, bool use_graph,
                     hipStream_t s, Step one_step) {
    if (!use_graph) {
        for (int i = 0; i < n; ++i) one_step(s);
        return 0;
    }
    int G = (int)opt_of(h, "graph_steps", 8);
    if (G < 1) G = 1;
    if (G > n) G = n;
    if (k.graph && (memcmp(key, k.key, sizeof k.key) != 0 || k.seed != seed || k.graph_steps != G)) {
        hipGraphExecDestroy(k.graph); k.graph = nullptr;
    }
    if (!k.graph) {
        hipGraph_t g = nullptr;
        hipError_t err = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
        if (err != hipSuccess) return fail(h, CMDGEN_EHIP, "hipStreamBeginCapture: %s", hipGetErrorString(err));
        for (int i = 0; i < G; ++i) one_step(s);
        err = hipStreamEndCapture(s, &g);                // always: a capture left open poisons every later launch on s
        if (err == hipSuccess) err = hipGraphInstantiate(&k.graph, g, nullptr, nullptr, 0);
        if (g) hipGraphDestroy(g);
        if (err != hipSuccess) { k.graph = nullptr; return fail(h, CMDGEN_EHIP, "capturing the chain's steps: %s", hipGetErrorString(err)); }
        memcpy(k.key, key, sizeof k.key); k.seed = seed; k.graph_steps = G;
    }
    for (int i = 0; i < n / G; ++i) HIPCHK(h, hipGraphLaunch(k.graph, s));
    for (int i = 0; i < n % G; ++i) one_step(s);
    return 0;
}

// the end of a chain: its launch errors, and the caller's later work ordered after it when it ran on the handle's own stream
static int end_chain(cmdgen_handle* h, hipStream_t caller, hipStream_t s) {
    HIPCHK(h, hipGetLastError());
    if (s != caller) {
        HIPCHK(h, hipEventRecord(h->ev_out, s));
        HIPCHK(h, hipStreamWaitEvent(caller, h->ev_out, 0));
    }
    return CMDGEN_OK;
}

// The parts a kind's ChainAlloc composes; each fills its member of the slot.  slot_alloc: `count` zeroed T in the slot's pool
template <class T>
static int slot_alloc(cmdgen_handle* h, ChainSlot& k, T*& dst, size_t count) {
    void* p; const int rc = dev_alloc(h, k.allocs, &p, count * sizeof(T), true);
    if (!rc) dst = (T*)p;
    return rc;
}
// a conditional chain's z and pocket (ChainBuf) and its pocket cache; coef: its posterior rows
static int alloc_chain_buf(cmdgen_handle* h, ChainSlot& k, const float* coef) {
    ChainBuf& c = k.buf;
    c.coef = (const float4*)coef; c.check = k.check; c.state = k.state;
    int rc = slot_alloc(h, k, c.z_phar, (size_t)h->lay.Nl * (3 + h->dims.P)); if (rc) return rc;
    rc = slot_alloc(h, k, c.xh_pocket, (size_t)h->lay.Np * (3 + h->dims.R)); if (rc) return rc;
    return alloc_pocket_cache(h, k);
}
// the edit kinds' InpaintBuf: coef2 | iop (n_steps rows each) at `coef2` in the table block, the known rows and marks, the offset per sample
static int alloc_inpaint_part(cmdgen_handle* h, ChainSlot& k, const float* coef2, int n_steps) {
    InpaintBuf& ip = k.inp;
    ip.coef2 = (const float4*)coef2;
    ip.iop = (const int4*)(coef2 + (size_t)n_steps * 4);
    ip.n_steps = n_steps;
    int rc = slot_alloc(h, k, ip.known, (size_t)h->lay.Nl * (3 + h->dims.P)); if (rc) return rc;    // (Nl bounds the unique rows of any grouping)
    rc = slot_alloc(h, k, ip.fix, (size_t)h->lay.Nl); if (rc) return rc;
    return slot_alloc(h, k, ip.poff, (size_t)h->lay.B);
}
// the restrained kinds' RestrainBuf: the guidance tail append_guidance packed at `guide` in the table block (n_rows guide rows), and com(P_in)
// (n_owners: the samples of the layout, or the groups of the restrained multi-pocket chain - the CSR offsets are [n_owners + 1])
static int alloc_restrain_part(cmdgen_handle* h, ChainSlot& k, const float* guide, int n_rows, int n_owners) {
    RestrainBuf& rb = k.restr;
    const float* par = guide + (size_t)n_rows * 4;
    rb.sa = (const float4*)guide;
    rb.clash_r = par[0]; rb.clash_k = par[1]; rb.scale = par[2]; rb.max_shift = par[3]; rb.guide_below = par[4];
    rb.rstart = (const int*)(par + 8);
    rb.rec = (const RestraintRec*)(par + 8 + (size_t)n_owners + 1);
    rb.op_energy = nullptr;
    return slot_alloc(h, k, rb.pin_com, (size_t)h->lay.B);
}
// the scoring kinds' ScoreBuf: the clean rows the levels noise
static int alloc_score_part(cmdgen_handle* h, ChainSlot& k) {
    const int rc = slot_alloc(h, k, k.score.xh0, (size_t)h->lay.Nl * (3 + h->dims.P)); if (rc) return rc;
    return slot_alloc(h, k, k.score.pocket0, (size_t)h->lay.Np * 3);
}
// the multi-pocket kinds' GroupTab: the group tables append_group_tables packed at `g` in the table block (the counts G, Nu come per call: group_tab)
static void point_group_tab(GroupTab& gt, const float* g, size_t B) {
    gt.first = (const int*)g; gt.size = (const int*)(g + B); gt.ubase = (const int*)(g + 2 * B);
    gt.weight = g + 3 * B; gt.group_first = (const int*)(g + 4 * B);
}
// the diverse kind's DiverseBuf: the tail append_sets packed at `g` in the table block (n_rows guide rows), com(P_in) and the buffers its
// launches hand on
static int alloc_diverse_part(cmdgen_handle* h, ChainSlot& k, const float* g, int n_rows) {
    DiverseBuf& db = k.div;
    const size_t B = (size_t)h->lay.B;
    const float* par = g + (size_t)n_rows * 4;
    db.sa = (const float4*)g;
    db.strength = par[0]; db.width = par[1]; db.inv2w2 = par[2]; db.max_shift = par[3]; db.guide_below = par[4];
    const int* tab = (const int*)(par + 8);
    db.set_first = tab; db.set_size = tab + B; db.set_row0 = tab + 2 * B; db.set_rows = tab + 3 * B;
    db.op_overlap = nullptr;
    int rc = slot_alloc(h, k, db.pin_com, B); if (rc) return rc;
    rc = slot_alloc(h, k, db.y, (size_t)h->lay.Nl * 3); if (rc) return rc;
    rc = slot_alloc(h, k, db.gd, (size_t)h->lay.Nl * 3); if (rc) return rc;
    return slot_alloc(h, k, db.po, (size_t)h->lay.Nl);
}
// The ChainAlloc of the ten sampling kinds: the ChainBuf, then the part of every section the body appended to its table block; the
// restrained multi-pocket kinds also get the displacement buffer their guide launch hands to their step launch.
static int alloc_sampling(cmdgen_handle* h, ChainSlot& k, const TableBlock& t, const float* dev, int n_steps) {
    int rc = alloc_chain_buf(h, k, dev); if (rc) return rc;
    if (t.edit) { rc = alloc_inpaint_part(h, k, dev + t.edit, n_steps); if (rc) return rc; }
    if (t.groups) point_group_tab(k.groups, dev + t.groups, (size_t)h->lay.B);
    if (t.guide) { rc = alloc_restrain_part(h, k, dev + t.guide, t.guide_rows, t.owners); if (rc) return rc; }
    if (t.sets) { rc = alloc_diverse_part(h, k, dev + t.sets, t.guide_rows); if (rc) return rc; }
    if (t.groups && t.guide) return slot_alloc(h, k, k.guide_d, (size_t)h->lay.Nl * 3);    // (Nl bounds the unique rows of any grouping)
    return 0;
}
// The ChainAlloc of the two scoring kinds: the ChainBuf (coef: one row per level, then the (alpha_T, sigma_T) row), the group tables where
// the block has them, the clean rows
static int alloc_scoring(cmdgen_handle* h, ChainSlot& k, const TableBlock& t, const float* dev, int) {
    const int rc = alloc_chain_buf(h, k, dev); if (rc) return rc;
    if (t.groups) point_group_tab(k.groups, dev + t.groups, (size_t)h->lay.B);
    return alloc_score_part(h, k);
}

// One chain call between begin_chain and end_chain: the stream it runs on, its slot, the launch description of its evaluations and, for
// the eleven conditional kinds, the slot's ChainBuf completed with the call's pointers.
struct Chain {
    cmdgen_handle* h = nullptr;
    ChainSlot* k = nullptr;
    hipStream_t caller = nullptr, s = nullptr;
    bool use_graph = false;
    EvalLaunch a, a2;                // evaluation 0 | the evaluations behind a step kernel, which ran pass 1 of the radius graph
    ChainBuf c{};

    int open(cmdgen_handle* h_, ChainKind kind, TableBlock& tables, int n_steps, ChainAlloc alloc, const int64_t* ids_host,
             const float* noise, unsigned long long seed, float* z_steps, float* pocket_steps, bool graph, cmdgen_stream stream) {
        h = h_; k = &h->chains[kind]; caller = (hipStream_t)stream; use_graph = graph;
        const int rc = begin_chain(h, kind, tables, n_steps, alloc, ids_host, use_graph, caller, &s, &a); if (rc) return rc;
        c = k->buf;
        c.noise = noise; c.seed = seed; c.z_steps = z_steps; c.pocket_steps = pocket_steps;
        return 0;
    }
    void eval(const EvalLaunch& e, hipStream_t ss) const {
        cmdgen_launch_eval(e, c.z_phar, c.xh_pocket, nullptr, c.coef, c.state, h->work.eps_tmp, nullptr, ss, nullptr);
    }
    // behind the kind's init launches: the pocket cache, then evaluation 0 (t of the chain's first row) - a scoring chain has none
    void start(bool eval0) {
        build_pocket_cache(h, *k, c, a, s);
        a2 = a;
        a2.skip_count = 1;                           // (pass 2 of the graph on a side stream was measured and dropped: the fork / join costs ~23 us per
                                                     // step inside the replayed graph, far more than the 10 us it hides; profiles/r02_b_step_fusion.txt)
        if (eval0) eval(a, s);
    }
    // n x (the kind's step launch, the evaluation at the new state); ptrs: the caller's pointers the captured steps bake in
    template <class Step>
    int steps(const void* const (&ptrs)[5], int n, Step step) {
        const void* key[6] = {ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], s};
        return run_steps(h, *k, key, c.seed, n, use_graph, s, [&](hipStream_t ss) { step(ss); eval(a2, ss); });
    }
    int close() { return end_chain(h, caller, s); }
};

// ---------------------------------------------------------------------------------
// the parts of the sampling chains, each with its plan (checked) and its section of the slot's table block.  The block of a kind is: the
// posterior rows, or with GIVEN rows the edit plan's tables (coef | coef2 | iop) | with GROUPS the group tables | the tail of the steering
// part, on a row boundary: the GUIDE's (kernels_restrain.hip holds the definition: a guidance term in the mean of every posterior op, or
// with given rows in op A; once per sample, or with groups once per group on the shared latent) or the SETS' (kernels_diverse.hip: a term
// that pushes the samples of a set apart), or the guide's and then the sets' (both heads hold the same guide rows).  Whatever changes a part therefore prepares the slot again and drops its captured steps.
// ---------------------------------------------------------------------------------
static_assert(sizeof(cmdgen_restraint) == sizeof(RestraintRec) && sizeof(RestraintRec) == 10 * sizeof(float), "the public record is the kernels'");
static_assert(CMDGEN_RESTRAINT_POSITION == RK_POSITION && CMDGEN_RESTRAINT_DISTANCE == RK_DISTANCE && CMDGEN_RESTRAINT_EXCLUSION == RK_EXCLUSION &&
              CMDGEN_MAX_RESTRAINTS == MAX_RESTRAINTS, "the public constants and the kernels' agree");

// sigma_t, alpha_t of every posterior op (rows s = K-1 .. 0, t = s + 1), fp32 as build_step_table evaluates its own (en_diffusion.py:859-867)
static void build_guide_table(const std::vector<float>& gamma, int T, int K, std::vector<float>& sa) {
    sa.assign((size_t)K * 2, 0.f);
    for (int i = 0; i < K; ++i) {
        const float t_arr = (float)(K - i) / (float)K;
        const float g_t = gamma[(size_t)lrintf(t_arr * (float)T)];
        sa[i * 2 + 0] = sqrtf(sigmoid_h(g_t));
        sa[i * 2 + 1] = sqrtf(sigmoid_h(-g_t));
    }
}

extern "C" int cmdgen_set_guide_table(cmdgen_handle* h, int32_t K, const float* sigma_alpha_host) {
    if (!h || K < 1 || !sigma_alpha_host) return fail(h, CMDGEN_EINVAL, "bad guide table");
    h->user_guide.assign(sigma_alpha_host, sigma_alpha_host + (size_t)K * 2);
    h->user_guide_K = K;
    return CMDGEN_OK;
}

// the op -> level map of a chain without jumps, for append_guide_rows: op i of K goes to level K - 1 - i
static std::vector<int> levels_down(int K) {
    std::vector<int> s_of((size_t)K);
    for (int i = 0; i < K; ++i) s_of[(size_t)i] = K - 1 - i;
    return s_of;
}

// The head of a steering tail (the guide's or the sets'), on a row boundary (group tables in front of it are padded to four floats): one
// guide row (sigma_t, alpha_t, 0, 0) per op, s_of[i] the level op i goes to (t = s + 1), then `spare` unused rows | par5, then 0, 0, 0 |
// `behind` zeroed floats for the part's own tables.  Records the rows in t.guide_rows -> the offset of the tail, and of what lies behind
static size_t append_guide_rows(const cmdgen_handle* h, TableBlock& t, int K, const std::vector<int>& s_of, int spare, const float (&par5)[5],
                                size_t behind, size_t* own) {
    std::vector<float> sa;                           // [K][2], row K - 1 - s for the op that goes to level s
    if (h->user_guide_K == K) sa = h->user_guide; else build_guide_table(h->gamma, h->cfg.timesteps, K, sa);
    const size_t c0 = (t.f.size() + 3) / 4 * 4, n_rows = s_of.size() + (size_t)spare;
    t.guide_rows = (int)n_rows;
    t.f.resize(c0 + n_rows * 4 + 8 + behind, 0.f);
    float* g = t.f.data() + c0;
    for (size_t i = 0; i < s_of.size(); ++i) {
        const size_t row = (size_t)(K - 1 - s_of[i]);
        g[4 * i] = sa[2 * row]; g[4 * i + 1] = sa[2 * row + 1];
    }
    memcpy(g + n_rows * 4, par5, sizeof par5);
    *own = c0 + n_rows * 4 + 8;
    return c0;
}

// ---- the groups part: one latent per GROUP of consecutive samples (kernels_multi.hip; the ops, the draw layout and the Philox counters
// are in include/cmdgen_hip.h).  The evaluations are the ordinary ones over the member samples.
static_assert(CMDGEN_MAX_GROUP == MAX_GROUP, "the public bound and the kernels' agree");

// the group tables of a call, per member (GroupTab), checked: what the sampling and the scoring chains with groups refuse alike
struct GroupPlan {
    std::vector<int> first, size, ubase, gfirst;
    std::vector<int64_t> gid;
    int G = 0; int64_t Nu = 0;
};
static int build_group_plan(cmdgen_handle* h, int64_t n_groups, const int64_t* group_size_host, const float* weight_host,
                            const int64_t* group_ids_host, GroupPlan& p) {
    const int B = h->lay.B;
    if (n_groups < 1 || n_groups > B) return fail(h, CMDGEN_EINVAL, "n_groups=%lld must be in [1, batch=%d]", (long long)n_groups, B);
    const int G = (int)n_groups;
    p.first.resize(B); p.size.resize(B); p.ubase.resize(B); p.gfirst.resize(G); p.gid.resize(B);
    int64_t members = 0, Nu = 0;
    for (int g = 0; g < G; ++g) {
        const int64_t M = group_size_host[g];
        if (M < 1 || M > CMDGEN_MAX_GROUP) return fail(h, CMDGEN_EINVAL, "group %d has %lld members: sizes must be in [1, %d]", g, (long long)M, CMDGEN_MAX_GROUP);
        if (members + M > B) { members += M; continue; }                 // (reported below with the sum)
        p.gfirst[g] = (int)members;
        double wsum = 0.0;
        for (int m = 0; m < (int)M; ++m) {
            const int b = (int)members + m;
            if (h->cur_nphar[b] != h->cur_nphar[members])
                return fail(h, CMDGEN_EINVAL, "group %d: member %d has %lld phar nodes, member 0 has %lld (the members of a group share one latent)",
                            g, m, (long long)h->cur_nphar[b], (long long)h->cur_nphar[members]);
            const float w = weight_host[b];
            if (!std::isfinite(w) || w < 0.f) return fail(h, CMDGEN_EINVAL, "group %d: weight %d is %g (weights must be finite and >= 0)", g, m, (double)w);
            wsum += (double)w;
            p.first[b] = (int)members; p.size[b] = (int)M; p.ubase[b] = (int)Nu;
            p.gid[b] = group_ids_host ? group_ids_host[g] : g;
        }
        if (std::fabs(wsum - 1.0) > 1e-5)
            return fail(h, CMDGEN_EINVAL, "group %d: its weights sum to %.9g, not 1 (the caller normalises them)", g, wsum);
        Nu += h->cur_nphar[members];
        members += M;
    }
    if (members != B) return fail(h, CMDGEN_EINVAL, "the group sizes sum to %lld, the layout has %d samples", (long long)members, B);
    if (plan_step_lds(h->lay.max_n, h->dims.P) > 64 * 1024)
        return fail(h, CMDGEN_EINVAL, "a sample has %d nodes: the multi-pocket step keeps a sample's positions, degrees and z in LDS (64 KiB)", h->lay.max_n);
    p.G = G; p.Nu = Nu;
    return 0;
}
// ... appended to a plan's tables: first | size | ubase | weight (one entry per member each), then the groups' first members
static void append_group_tables(TableBlock& t, const GroupPlan& p, const float* weight_host, int B) {
    const size_t c0 = t.f.size();
    t.groups = c0; t.G = p.G;
    t.f.resize(c0 + (size_t)4 * B + p.G);
    float* g = t.f.data() + c0;
    memcpy(g, p.first.data(), (size_t)B * sizeof(int)); memcpy(g + B, p.size.data(), (size_t)B * sizeof(int));
    memcpy(g + 2 * (size_t)B, p.ubase.data(), (size_t)B * sizeof(int)); memcpy(g + 3 * (size_t)B, weight_host, (size_t)B * sizeof(float));
    memcpy(g + 4 * (size_t)B, p.gfirst.data(), (size_t)p.G * sizeof(int));
}
// the slot's group tables with the call's counts
static GroupTab group_tab(const ChainSlot& k, const GroupPlan& p) { GroupTab gt = k.groups; gt.G = p.G; gt.Nu = (int)p.Nu; return gt; }

// ---- the guide part: restraints, owned (cmdgen_restraint::sample) by the layout's samples or, in a call with groups, by its groups
// The restraint arguments of a restrained chain, checked (gp: the call's groups, or null; par5: clash_radius, clash_k, scale, max_shift,
// guide_below; step_lds: the step kernel's LDS for this layout - 0 with groups, where the step keeps its unguided parent's LDS, which
// build_group_plan has checked, and the guide kernel less).  rstart [owners + 1]: the CSR offsets, rec: the records sorted by owner, the
// fields a kind does not read zeroed
static int check_restraints(cmdgen_handle* h, const GroupPlan* gp, const cmdgen_restraint* restraints_host, int64_t n_restraints,
                            const float (&par5)[5], size_t step_lds, std::vector<int>& rstart, std::vector<cmdgen_restraint>& rec) {
    const float clash_radius = par5[0], clash_k = par5[1], scale = par5[2], max_shift = par5[3], guide_below = par5[4];
    const char *one = "sample", *whose = "the layout's";
    std::vector<long long> nphar(h->cur_nphar.begin(), h->cur_nphar.end());          // points of every owner
    if (gp) {
        one = "group"; whose = "the call's";
        nphar.clear();
        for (int g = 0; g < gp->G; ++g) nphar.push_back((long long)h->cur_nphar[(size_t)gp->gfirst[g]]);
    }
    if (n_restraints < 0 || (n_restraints > 0 && !restraints_host)) return fail(h, CMDGEN_EINVAL, "n_restraints=%lld without a restraint list", (long long)n_restraints);
    auto ok = [](float v) { return std::isfinite(v) && v >= 0.f; };
    if (!ok(clash_radius) || !ok(clash_k)) return fail(h, CMDGEN_EINVAL, "clash_radius=%g, clash_k=%g must be finite and >= 0", (double)clash_radius, (double)clash_k);
    if (!ok(scale)) return fail(h, CMDGEN_EINVAL, "scale=%g must be finite and >= 0", (double)scale);
    if (!(std::isfinite(max_shift) && max_shift > 0.f)) return fail(h, CMDGEN_EINVAL, "max_shift=%g must be finite and > 0", (double)max_shift);
    if (!(guide_below >= 0.f && guide_below <= 1.f)) return fail(h, CMDGEN_EINVAL, "guide_below=%g must be in [0, 1]", (double)guide_below);
    const int B = (int)nphar.size();
    rstart.assign((size_t)B + 1, 0);
    for (int64_t r = 0; r < n_restraints; ++r) {
        const cmdgen_restraint& q = restraints_host[r];
        const long long ri = (long long)r;
        if (q.kind != RK_POSITION && q.kind != RK_DISTANCE && q.kind != RK_EXCLUSION) return fail(h, CMDGEN_EINVAL, "restraint %lld: unknown kind %d", ri, q.kind);
        if (q.sample < 0 || q.sample >= B) return fail(h, CMDGEN_EINVAL, "restraint %lld: %s %d outside %s %d %ss", ri, one, q.sample, whose, B, one);
        const long long nl = nphar[(size_t)q.sample];
        if (q.kind != RK_EXCLUSION && (q.i < 0 || q.i >= nl)) return fail(h, CMDGEN_EINVAL, "restraint %lld: point %d, %s %d has %lld points", ri, q.i, one, q.sample, nl);
        if (q.kind == RK_DISTANCE) {
            if (q.j < 0 || q.j >= nl) return fail(h, CMDGEN_EINVAL, "restraint %lld: point %d, %s %d has %lld points", ri, q.j, one, q.sample, nl);
            if (q.i == q.j) return fail(h, CMDGEN_EINVAL, "restraint %lld: a distance between point %d and itself (i == j)", ri, q.i);
            if (!ok(q.a) || !ok(q.b)) return fail(h, CMDGEN_EINVAL, "restraint %lld: lo=%g, hi=%g must be finite and >= 0", ri, (double)q.a, (double)q.b);
            if (q.a > q.b) return fail(h, CMDGEN_EINVAL, "restraint %lld: lo=%g > hi=%g", ri, (double)q.a, (double)q.b);
        } else {
            if (!ok(q.a)) return fail(h, CMDGEN_EINVAL, "restraint %lld: radius=%g must be finite and >= 0", ri, (double)q.a);
            if (!std::isfinite(q.c[0]) || !std::isfinite(q.c[1]) || !std::isfinite(q.c[2])) return fail(h, CMDGEN_EINVAL, "restraint %lld: a non-finite centre", ri);
        }
        if (!ok(q.k)) return fail(h, CMDGEN_EINVAL, "restraint %lld: k=%g must be finite and >= 0", ri, (double)q.k);
        if (++rstart[(size_t)q.sample + 1] > CMDGEN_MAX_RESTRAINTS)
            return fail(h, CMDGEN_EINVAL, "%s %d has more than %d restraints", one, q.sample, CMDGEN_MAX_RESTRAINTS);
    }
    if (step_lds > PLAN_RESTRAINED_LDS_MAX)
        return fail(h, CMDGEN_EINVAL, "a sample has %d nodes: the restrained step keeps a sample's positions, z and guidance terms in LDS (64 KiB)", h->lay.max_n);
    for (int b = 0; b < B; ++b) rstart[(size_t)b + 1] += rstart[b];
    rec.assign((size_t)n_restraints, cmdgen_restraint{});
    {
        std::vector<int> at(rstart.begin(), rstart.end() - 1);
        for (int64_t r = 0; r < n_restraints; ++r) {             // stable: an owner's restraints keep their list order
            cmdgen_restraint q = restraints_host[r];
            if (q.kind == RK_EXCLUSION) { q.i = 0; q.j = 0; }
            if (q.kind == RK_POSITION) q.j = 0;
            if (q.kind != RK_DISTANCE) q.b = 0.f;
            if (q.kind == RK_DISTANCE) q.c[0] = q.c[1] = q.c[2] = 0.f;
            rec[(size_t)at[q.sample]++] = q;                     // (fields a kind does not read are zeroed: they are part of the slot's key)
        }
    }
    return 0;
}
// The guidance tail of a table block: append_guide_rows' head | rstart [owners + 1] | rec.  alloc_restrain_part points a RestrainBuf at it.
static void append_guidance(const cmdgen_handle* h, TableBlock& t, int K, const std::vector<int>& s_of, int spare, const float (&par5)[5],
                            const std::vector<int>& rstart, const std::vector<cmdgen_restraint>& rec) {
    size_t own;
    t.guide = append_guide_rows(h, t, K, s_of, spare, par5, rstart.size() + rec.size() * 10, &own);
    t.owners = (int)rstart.size() - 1;
    float* const csr = t.f.data() + own;
    memcpy(csr, rstart.data(), rstart.size() * sizeof(int));
    if (!rec.empty()) memcpy(csr + rstart.size(), rec.data(), rec.size() * sizeof(cmdgen_restraint));
}

// ---- the sets part: the layout's samples partitioned into SETS of consecutive samples, "the draws for one pocket" (DiverseBuf).  The tail is:
// the guide rows (sigma_t, alpha_t, 0, 0; K + 1 of them, the last unused) | strength, width, 1 / (2 w^2), max_shift, guide_below, 0, 0, 0 |
// per sample set_first, set_size, set_row0, set_rows
static_assert(CMDGEN_MAX_SET_ROWS == MAX_SET_ROWS, "the public bound and the kernels' agree");

// the scalars and the set tables of a call, per sample, checked
struct SetPlan { std::vector<int> first, size, row0, rows; };
static int build_set_plan(cmdgen_handle* h, int64_t n_sets, const int64_t* set_size_host, float strength, float width, float max_shift,
                          float guide_below, SetPlan& p) {
    if (!(std::isfinite(strength) && strength >= 0.f)) return fail(h, CMDGEN_EINVAL, "strength=%g must be finite and >= 0", (double)strength);
    if (!(std::isfinite(width) && width > 0.f)) return fail(h, CMDGEN_EINVAL, "width=%g must be finite and > 0", (double)width);
    if (!(std::isfinite(max_shift) && max_shift > 0.f)) return fail(h, CMDGEN_EINVAL, "max_shift=%g must be finite and > 0", (double)max_shift);
    if (!(guide_below >= 0.f && guide_below <= 1.f)) return fail(h, CMDGEN_EINVAL, "guide_below=%g must be in [0, 1]", (double)guide_below);
    const int B = h->lay.B;
    if (n_sets < 1 || n_sets > B) return fail(h, CMDGEN_EINVAL, "n_sets=%lld must be in [1, batch=%d]", (long long)n_sets, B);
    p.first.resize(B); p.size.resize(B); p.row0.resize(B); p.rows.resize(B);
    int64_t members = 0, row = 0;
    for (int64_t g = 0; g < n_sets; ++g) {
        const int64_t M = set_size_host[g];
        if (M < 1) return fail(h, CMDGEN_EINVAL, "set_size[%lld]=%lld: every set has at least one sample", (long long)g, (long long)M);
        if (members + M > B) { members += M; continue; }                 // (reported below with the sum)
        int64_t rows = 0;
        for (int64_t m = 0; m < M; ++m) rows += h->cur_nphar[(size_t)(members + m)];
        if (rows > CMDGEN_MAX_SET_ROWS)
            return fail(h, CMDGEN_EINVAL, "set_size[%lld]: the set has %lld phar rows, at most %d (the pair launch costs rows^2)", (long long)g,
                        (long long)rows, CMDGEN_MAX_SET_ROWS);
        for (int64_t m = 0; m < M; ++m) {
            const size_t b = (size_t)(members + m);
            p.first[b] = (int)members; p.size[b] = (int)M; p.row0[b] = (int)row; p.rows[b] = (int)rows;
        }
        members += M; row += rows;
    }
    if (members != B) return fail(h, CMDGEN_EINVAL, "set_size sums to %lld, the layout has %d samples", (long long)members, B);
    if (plan_step_lds(h->lay.max_n, h->dims.P) > 64 * 1024)
        return fail(h, CMDGEN_EINVAL, "a sample has %d nodes: the diverse step keeps a sample's positions, degrees and z in LDS (64 KiB)", h->lay.max_n);
    return 0;
}
// The sets' tail of a table block: append_guide_rows' head (K guide rows and one unused) | the four set tables, B entries each.
// alloc_diverse_part points a DiverseBuf at it.
static void append_sets(const cmdgen_handle* h, TableBlock& t, int K, const float (&par5)[5], const SetPlan& p) {
    const size_t B = p.first.size();
    size_t own;
    t.sets = append_guide_rows(h, t, K, levels_down(K), 1, par5, 4 * B, &own);
    float* tab = t.f.data() + own;
    memcpy(tab, p.first.data(), B * sizeof(int)); memcpy(tab + B, p.size.data(), B * sizeof(int));
    memcpy(tab + 2 * B, p.row0.data(), B * sizeof(int)); memcpy(tab + 3 * B, p.rows.data(), B * sizeof(int));
}

// ---------------------------------------------------------------------------------
// joint model: EnVariationalDiffusion.sample / .inpaint (en_diffusion.py:576-831)
// ---------------------------------------------------------------------------------
// get_repaint_schedule (en_diffusion.py:649-670): denoising steps to run before each jump back
static std::vector<int> repaint_schedule(int resamplings, int jump_length, int timesteps) {
    std::vector<int> sched;
    int curr_t = 0;
    while (curr_t < timesteps) {
        if (curr_t + jump_length < timesteps) {
            if (!sched.empty()) {
                sched.back() += jump_length;
                for (int i = 0; i < resamplings - 1; ++i) sched.push_back(jump_length);
            } else {
                for (int i = 0; i < resamplings; ++i) sched.push_back(jump_length);
            }
            curr_t += jump_length;
        } else {
            const int residual = timesteps - curr_t;
            if (!sched.empty()) sched.back() += residual; else sched.push_back(residual);
            curr_t += residual;
        }
    }
    return std::vector<int>(sched.rbegin(), sched.rend());
}

struct JointPlan {
    std::vector<float> coef, coef2;     // [n_steps+1][4], [n_steps+1][4]
    std::vector<int> iop;               // [n_steps+1][4]
    int n_steps = 0, n_draws = 0;
};

// The op table of one chain: one row per network evaluation, in execution order (the walk of :723-813).
static JointPlan build_joint_plan(const std::vector<float>& gamma, int T, int K, int resamplings, int jump, bool inpaint) {
    JointPlan p;
    const std::vector<int> sched = inpaint ? repaint_schedule(resamplings, jump, K) : std::vector<int>{K};
    auto g_at = [&](int step) { return gamma[(size_t)lrintf(((float)step / (float)K) * (float)T)]; };
    int draw = 1;                       // draw 0 = z_T
    int s = K - 1;
    for (size_t i = 0; i < sched.size(); ++i) {
        for (int j = 0; j < sched[i]; ++j) {
            const float g_s = g_at(s), g_t = g_at(s + 1);
            const float sigma2_ts = -expm1f(softplus_f(g_s) - softplus_f(g_t));
            const float alpha_ts = expf(0.5f * (logsigmoid_f(-g_t) - logsigmoid_f(-g_s)));
            const float sigma_ts = sqrtf(sigma2_ts);
            const float sigma_s = sqrtf(sigmoid_h(g_s)), sigma_t = sqrtf(sigmoid_h(g_t));
            p.coef.insert(p.coef.end(), {alpha_ts, sigma2_ts / alpha_ts / sigma_t, sigma_ts * sigma_s / sigma_t,
                                         (float)(s + 1) / (float)K});
            float re_a = 0.f, re_s = 0.f; int flags = 0;
            const int draw0 = draw;
            draw += inpaint ? 2 : 1;
            if (j == sched[i] - 1 && i + 1 < sched.size()) {      // jump back s -> s + jump_length
                const float g_t2 = g_at(s + jump);
                re_s = sqrtf(-expm1f(softplus_f(g_s) - softplus_f(g_t2)));
                re_a = expf(0.5f * (logsigmoid_f(-g_t2) - logsigmoid_f(-g_s)));
                flags = 1; draw += 1;
                s = s + jump;
            }
            p.coef2.insert(p.coef2.end(), {sqrtf(sigmoid_h(-g_s)), sigma_s, re_a, re_s});
            p.iop.insert(p.iop.end(), {flags, draw0, 0, 0});
            s -= 1;
            p.n_steps += 1;
        }
    }
    const float g0 = gamma[0];
    p.coef.insert(p.coef.end(), {sqrtf(sigmoid_h(g0)), sqrtf(sigmoid_h(-g0)), expf(0.5f * g0), 0.f});
    p.coef2.insert(p.coef2.end(), {0.f, 0.f, 0.f, 0.f});
    p.iop.insert(p.iop.end(), {0, draw, 0, 0});
    p.n_draws = draw + 1;
    return p;
}

static int check_joint_args(cmdgen_handle* h, int K, int resamplings, int jump) {
    if (!h->dims.joint) return fail(h, CMDGEN_ESTATE, "joint chains need a handle created with update_pocket_coords=1");
    const int rc = check_timesteps(h, K); if (rc) return rc;
    if (resamplings < 1 || jump < 1) return fail(h, CMDGEN_EINVAL, "resamplings and jump_length must be >= 1");
    return 0;
}

extern "C" int cmdgen_joint_plan(cmdgen_handle* h, int32_t timesteps, int32_t resamplings, int32_t jump_length,
                                 int32_t inpaint, int64_t* n_steps, int64_t* n_draws) {
    if (!h) return CMDGEN_EINVAL;
    if (!h->finalized) return fail(h, CMDGEN_ESTATE, "weights not finalised (cmdgen_finalize_weights)");
    int rc = check_joint_args(h, timesteps, resamplings, jump_length); if (rc) return rc;
    const JointPlan p = build_joint_plan(h->gamma, h->cfg.timesteps, timesteps, resamplings, jump_length, inpaint != 0);
    if (n_steps) *n_steps = p.n_steps;
    if (n_draws) *n_draws = p.n_draws;
    return CMDGEN_OK;
}

// JointBuf: the plan's rows (coef, coef2, iop: n_steps + 1 each), the state, and the scratch of the combined draws
static int alloc_joint(cmdgen_handle* h, ChainSlot& k, const TableBlock&, const float* tables, int n_steps) {
    JointBuf& c = k.joint;
    c.coef = (const float4*)tables;
    c.coef2 = (const float4*)(tables + (size_t)(n_steps + 1) * 4);
    c.iop = (const int4*)(tables + (size_t)(n_steps + 1) * 8);
    c.check = k.check; c.state = k.state;
    const size_t np_ = (size_t)h->lay.Nl * (3 + h->dims.P), nq_ = (size_t)h->lay.Np * (3 + h->dims.R);
    float** const phar[] = {&c.z_phar, &c.e_phar, &c.zk_phar, &c.x0_phar};
    float** const pocket[] = {&c.z_pocket, &c.e_pocket, &c.zk_pocket, &c.x0_pocket};
    for (int i = 0; i < 4; ++i) {
        int rc = slot_alloc(h, k, *phar[i], np_); if (rc) return rc;
        rc = slot_alloc(h, k, *pocket[i], nq_); if (rc) return rc;
    }
    return slot_alloc(h, k, k.eps_pocket, nq_);
}

extern "C" int cmdgen_joint_chain(cmdgen_handle* h, const float* phar_x, const float* phar_onehot,
                                  const float* pocket_x, const float* pocket_onehot,
                                  const float* phar_fixed, const float* pocket_fixed,
                                  int32_t timesteps, int32_t resamplings, int32_t jump_length,
                                  const float* noise, int64_t n_draws, uint64_t seed, const int64_t* pocket_ids_host,
                                  float* xh_phar_out, float* xh_pocket_out, float* z_steps_out,
                                  int32_t use_graph, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    rc = check_joint_args(h, timesteps, resamplings, jump_length); if (rc) return rc;
    if (!xh_phar_out || !xh_pocket_out) return fail(h, CMDGEN_EINVAL, "null output pointer");
    const bool inpaint = phar_fixed != nullptr || pocket_fixed != nullptr;
    if (inpaint && (!phar_fixed || !pocket_fixed || !phar_x || !phar_onehot || !pocket_x || !pocket_onehot))
        return fail(h, CMDGEN_EINVAL, "inpainting needs phar_x, phar_onehot, pocket_x, pocket_onehot and both fixed masks");
    const JointPlan plan = build_joint_plan(h->gamma, h->cfg.timesteps, timesteps, resamplings, jump_length, inpaint);
    rc = check_draws(h, noise, n_draws, plan.n_draws, "combined draws"); if (rc) return rc;
    const int n_steps = plan.n_steps;
    TableBlock tables = plan_tables(plan.coef, plan.coef2, plan.iop);
    Chain ch;                                        // (open and close only: the joint chain has no ChainBuf and evaluates BEFORE its step)
    rc = ch.open(h, CHAIN_JOINT, tables, n_steps, alloc_joint, pocket_ids_host, noise, seed, z_steps_out, nullptr, use_graph, stream); if (rc) return rc;
    const Dims& d = h->dims;
    const hipStream_t s = ch.s;
    float* const eps_pocket = ch.k->eps_pocket;
    JointBuf c = ch.k->joint;
    c.fix_phar = phar_fixed; c.fix_pocket = pocket_fixed; c.z_steps = z_steps_out;
    c.seed = seed; c.noise = noise;
    cmdgen_launch_joint_init(h->lay, d, c, phar_x, phar_onehot, pocket_x, pocket_onehot, s);
    const void* key[6] = {noise, z_steps_out, nullptr, phar_fixed, pocket_fixed, s};
    rc = run_steps(h, *ch.k, key, seed, n_steps, use_graph, s, [&](hipStream_t ss) {
        cmdgen_launch_eval(ch.a, c.z_phar, c.z_pocket, nullptr, c.coef, c.state, h->work.eps_tmp, eps_pocket, ss, nullptr);
        cmdgen_launch_joint_step(h->lay, d, c, h->work.eps_tmp, eps_pocket, ss);
    });
    if (rc) return rc;
    cmdgen_launch_eval(ch.a, c.z_phar, c.z_pocket, nullptr, c.coef, c.state, h->work.eps_tmp, eps_pocket, s, nullptr);
    cmdgen_launch_joint_final(h->lay, d, c, h->work.eps_tmp, eps_pocket, xh_phar_out, xh_pocket_out, ch.k->cog, s);
    return ch.close();
}

// ---------------------------------------------------------------------------------
// the given part of the sampling chains, with its plan: conditional RePaint and the edit chain, ConditionalDDPM.inpaint / .edit
// (kernels_inpaint.hip; the op semantics and the draw scheme are in include/cmdgen_hip.h; with groups the ops run on the shared latent,
// kernels_multi.hip, the known rows and marks held once per group).  Inpainting is the edit chain with both masks equal and start = timesteps.
// ---------------------------------------------------------------------------------
struct InpaintPlan {
    std::vector<float> coef, coef2;     // [n_steps+1][4] (last: decode row), [n_steps][4]
    std::vector<int> iop;               // [n_steps][4]
    std::vector<int> s_of;              // [n_steps] the level s every op goes to (t = s + 1)
    int n_steps = 0, n_draws = 0;
    float alpha_start = 0.f, sigma_start = 0.f;     // q(z_start | x) of a chain that starts below t = T
};

// One row per op in execution order.  The posterior rows are the step table's (the caller's, when it supplied one for K:
// then an op at step s uses exactly the scalars cmdgen_sample_chain uses there).  The ops walk s = start-1 .. 0 on the K grid
// with get_repaint_schedule(resamplings, jump, start).
static InpaintPlan build_inpaint_plan(const cmdgen_handle* h, int K, int start, int resamplings, int jump) {
    InpaintPlan p;
    const std::vector<float> tab = step_table(h, K);
    const int T = h->cfg.timesteps;
    auto g_at = [&](int step) { return h->gamma[(size_t)lrintf(((float)step / (float)K) * (float)T)]; };
    const std::vector<int> sched = repaint_schedule(resamplings, jump, start);
    p.alpha_start = sqrtf(sigmoid_h(-g_at(start)));
    p.sigma_start = sqrtf(sigmoid_h(g_at(start)));
    int draw = 1;                       // row 0 = z_T (z_start)
    int s = start - 1;
    for (size_t i = 0; i < sched.size(); ++i) {
        for (int j = 0; j < sched[i]; ++j) {
            p.coef.insert(p.coef.end(), tab.begin() + (size_t)(K - 1 - s) * 4, tab.begin() + (size_t)(K - s) * 4);
            const float g_s = g_at(s);
            const int rowA = draw++, rowB = draw++;
            p.s_of.push_back(s);
            float re_a = 0.f, re_s = 0.f; int flags = 0, rowC = 0;
            if (j == sched[i] - 1 && i + 1 < sched.size()) {      // jump back s -> s + jump_length
                const float g_t2 = g_at(s + jump);
                re_s = sqrtf(-expm1f(softplus_f(g_s) - softplus_f(g_t2)));
                re_a = expf(0.5f * (logsigmoid_f(-g_t2) - logsigmoid_f(-g_s)));
                flags = 1; rowC = draw++;
                s = s + jump;
            }
            p.coef2.insert(p.coef2.end(), {sqrtf(sigmoid_h(-g_s)), sqrtf(sigmoid_h(g_s)), re_a, re_s});
            p.iop.insert(p.iop.end(), {flags, rowA, rowB, rowC});
            s -= 1;
            p.n_steps += 1;
        }
    }
    p.coef.insert(p.coef.end(), tab.begin() + (size_t)K * 4, tab.begin() + (size_t)(K + 1) * 4);
    p.n_draws = draw + 1;               // + the decode draw
    return p;
}

static int check_inpaint_args(cmdgen_handle* h, int K, int start, int resamplings, int jump) {
    if (h->dims.joint) return fail(h, CMDGEN_ESTATE, "this handle is the joint model (update_pocket_coords=1): use cmdgen_joint_chain");
    if (h->dims.no_com) return fail(h, CMDGEN_ESTATE, "inpainting is not supported for no_com_projection handles (SimpleConditionalDDPM)");
    const int rc = check_timesteps(h, K); if (rc) return rc;
    if (start < 1 || start > K) return fail(h, CMDGEN_EINVAL, "start=%d must be in [1, timesteps=%d]", start, K);
    if (resamplings < 1 || jump < 1) return fail(h, CMDGEN_EINVAL, "resamplings and jump_length must be >= 1");
    return 0;
}

extern "C" int cmdgen_edit_plan(cmdgen_handle* h, int32_t timesteps, int32_t start, int32_t resamplings, int32_t jump_length,
                                int64_t* n_steps, int64_t* n_draws) {
    if (!h) return CMDGEN_EINVAL;
    if (!h->finalized) return fail(h, CMDGEN_ESTATE, "weights not finalised (cmdgen_finalize_weights)");
    int rc = check_inpaint_args(h, timesteps, start, resamplings, jump_length); if (rc) return rc;
    const InpaintPlan p = build_inpaint_plan(h, timesteps, start, resamplings, jump_length);
    if (n_steps) *n_steps = p.n_steps;
    if (n_draws) *n_draws = p.n_draws;
    return CMDGEN_OK;
}

extern "C" int cmdgen_inpaint_plan(cmdgen_handle* h, int32_t timesteps, int32_t resamplings, int32_t jump_length,
                                   int64_t* n_steps, int64_t* n_draws) {
    return cmdgen_edit_plan(h, timesteps, timesteps, resamplings, jump_length, n_steps, n_draws);
}

// the decode draw of a plan is its last row; the final kernels read theirs from row 1 + n_steps of `noise`: `skip` rows further with an edit
// plan, 0 without one (rows: phar rows per draw)
static ChainBuf decode_buf(const ChainBuf& c, int skip, size_t rows, int P) {
    ChainBuf cf = c;
    if (c.noise) cf.noise = c.noise + (size_t)skip * rows * (3 + P);
    return cf;
}

// ---------------------------------------------------------------------------------
// the ten sampling chains: what an entry received (the part names are Handle._sampling_chain's and tests/chain_kit.run_chain's; a part
// the kind lacks is null), and their one body
// ---------------------------------------------------------------------------------
struct GroupsPart { int64_t n; const int64_t* size_host; const float* weight_host; };
struct GivenPart { const float *phar_x, *phar_onehot, *fix_x, *fix_h; int start, resamplings, jump_length; };      // the rows and their plan
struct GuidePart {
    const cmdgen_restraint* restraints_host; int64_t n;
    float par[5];                                    // clash_radius, clash_k, scale, max_shift, guide_below
    float *energy_out, *op_energy_out;
};
struct SetsPart { int64_t n; const int64_t* size_host; float strength, width, max_shift, guide_below; float *overlap_out, *op_overlap_out; };
struct SamplingCall {
    ChainKind kind;
    const char* name;                                // the kind's name as its refusal of a joint or no_com handle words it; null: the kind refuses the
                                                     // joint model alone, by pointing at cmdgen_joint_chain (with given rows check_inpaint_args refuses both)
    const char* no_com_why; int no_com_code;         // ... and what the kind adds for a no_com handle, with the code it returns
    const float *pocket_x, *pocket_onehot;
    int timesteps;
    const float* noise; int64_t n_draws;             // (n_draws is read with given rows only: without them the schedule has timesteps + 2 draws)
    uint64_t seed; const int64_t* ids_host;          // ids: of the pockets, or with groups of the groups
    float *xh_phar_out, *xh_pocket_out, *z_steps_out, *pocket_steps_out;
    int32_t use_graph; cmdgen_stream stream;
    const GroupsPart* groups; const GivenPart* given; const GuidePart* guide; const SetsPart* sets;
};
static const char* const kGuideFrame = ": the guidance frame follows the centre-of-mass projections";
static const char* const kEditGuideFrame = ": the edit chain and the guidance frame follow the centre-of-mass projections";

static int sampling_chain(cmdgen_handle* h, const SamplingCall& q) {
    const GroupsPart* const gr = q.groups; const GivenPart* const gv = q.given; const GuidePart* const gu = q.guide; const SetsPart* const se = q.sets;
    // ---- refusals: the handle, the pointers
    int rc = check_ready(h); if (rc) return rc;
    if (q.name) { rc = refuse_joint_no_com(h, q.name, kPocketDiffuses, q.no_com_why, q.no_com_code); if (rc) return rc; }
    else if (h->dims.joint) return fail(h, CMDGEN_ESTATE, "this handle is the joint model (update_pocket_coords=1): use cmdgen_joint_chain");
    bool missing = !q.pocket_x || !q.pocket_onehot || !q.xh_phar_out || !q.xh_pocket_out;
    const char* null_text = "null device pointer";
    if (gr) { missing |= !gr->size_host || !gr->weight_host; null_text = "null pointer"; }
    if (gv) missing |= !gv->phar_x || !gv->phar_onehot || !gv->fix_x || !gv->fix_h;
    if (gu) missing |= !gu->energy_out;
    if (se) {
        missing |= !se->size_host || !se->overlap_out;
        null_text = gu ? "null pointer (pocket_x, pocket_onehot, set_size_host, xh_phar_out, xh_pocket_out, energy_out and overlap_out are required)"
                       : "null pointer (pocket_x, pocket_onehot, set_size_host, xh_phar_out, xh_pocket_out and overlap_out are required)";
    }
    if (missing) return fail(h, CMDGEN_EINVAL, "%s", null_text);
    // ---- the plans of the parts present.  Without given rows the ops go down the K levels one by one, with one spare guide row; with them the
    // plan says where every op goes, how many there are and where the decode draw lies
    const int K = q.timesteps, P = h->dims.P;
    InpaintPlan plan; GroupPlan gp; SetPlan sp;
    std::vector<int> s_of, rstart; std::vector<cmdgen_restraint> rec;
    int n_steps = K, spare = 1, decode_skip = 0;
    size_t guide_lds;                                // the LDS of the guided step of this corner (check_restraints)
    if (gv) {
        rc = check_inpaint_args(h, K, gv->start, gv->resamplings, gv->jump_length); if (rc) return rc;
        plan = build_inpaint_plan(h, K, gv->start, gv->resamplings, gv->jump_length);
        rc = check_draws(h, q.noise, q.n_draws, plan.n_draws); if (rc) return rc;
        n_steps = plan.n_steps; s_of = plan.s_of; spare = 0; decode_skip = plan.n_draws - 1 - (1 + plan.n_steps);
        guide_lds = plan_restrained_edit_step_lds(h->lay.max_n, P);
    } else {
        rc = check_timesteps(h, K); if (rc) return rc;
        s_of = levels_down(K);
        guide_lds = se ? plan_diverse_restrained_step_lds(h->lay.max_n, P) : plan_restrained_step_lds(h->lay.max_n, P);
    }
    if (gr) {
        rc = build_group_plan(h, gr->n, gr->size_host, gr->weight_host, q.ids_host, gp); if (rc) return rc;
        guide_lds = 0;
    }
    if (gu) { rc = check_restraints(h, gr ? &gp : nullptr, gu->restraints_host, gu->n, gu->par, guide_lds, rstart, rec); if (rc) return rc; }
    if (se) { rc = build_set_plan(h, se->n, se->size_host, se->strength, se->width, se->max_shift, se->guide_below, sp); if (rc) return rc; }
    // ---- the table block: its tables, the known rows and the marks are slot buffers (a changed plan, start, grouping, weight, restraint,
    // partition or scalar prepares the slot again and drops its graph); the ids are uploaded per call, the caller's pointers are the graph's key
    TableBlock tables = gv ? plan_tables(plan.coef, plan.coef2, plan.iop) : posterior_rows(step_table(h, K));
    if (gr) append_group_tables(tables, gp, gr->weight_host, h->lay.B);
    if (gu) append_guidance(h, tables, K, s_of, spare, gu->par, rstart, rec);
    if (se) append_sets(h, tables, K, {se->strength, se->width, 1.0f / (2.0f * (se->width * se->width)), se->max_shift, se->guide_below}, sp);
    Chain ch;
    rc = ch.open(h, q.kind, tables, n_steps, alloc_sampling, gr ? gp.gid.data() : q.ids_host, q.noise, q.seed, q.z_steps_out, q.pocket_steps_out,
                 q.use_graph, q.stream);
    if (rc) return rc;
    const Layout& lay = h->lay; const Dims& d = h->dims; const Work& w = h->work;
    const ChainBuf& c = ch.c;
    float* const eps = w.eps_tmp;
    const hipStream_t s = ch.s;
    // the slot's buffer of every part, completed with the call's pointers (a part the kind lacks: its empty buffer, which nothing reads)
    const InpaintBuf ip = ch.k->inp;
    const GroupTab gt = group_tab(*ch.k, gp);
    RestrainBuf rb = ch.k->restr;
    DiverseBuf db = ch.k->div;
    float* const gd = ch.k->guide_d;
    float *op_side = nullptr, *op_side2 = nullptr;   // the steering parts' outputs per op: the fourth and the fifth pointer of the graph's key
    if (gu) op_side = rb.op_energy = gu->op_energy_out;
    if (se) { (gu ? op_side2 : op_side) = db.op_overlap = se->op_overlap_out; rb.pin_com = db.pin_com; }   // (k_restrain_prep fills pin_com and reads nothing else
                                                                                                           // of rb; with both parts they read the one buffer)
    // ---- init: z_T around the (weighted) pocket centre, or part-way z ~ q(z_start | the given rows); the known rows and marks; com(P_in)
    const bool from_prior = !gv || gv->start == K;
    if (gr) {
        if (from_prior) cmdgen_launch_multi_init(lay, d, c, gt, q.pocket_x, q.pocket_onehot, s);
        else cmdgen_launch_multi_edit_start(lay, d, c, gt, plan.alpha_start, plan.sigma_start, gv->phar_x, gv->phar_onehot, q.pocket_x, q.pocket_onehot, s);
        // a launch of its own after the init: every member reads the projected pocket of its group's FIRST member for the offset
        if (gv) cmdgen_launch_multi_edit_prep(lay, d, c, gt, ip, gv->phar_x, gv->phar_onehot, gv->fix_x, gv->fix_h, q.pocket_x, s);
    } else {
        if (from_prior) cmdgen_launch_chain_init(lay, d, c, q.pocket_x, q.pocket_onehot, s);
        else cmdgen_launch_edit_start(lay, d, c, ip, plan.alpha_start, plan.sigma_start, gv->phar_x, gv->phar_onehot, gv->fix_x, gv->fix_h, q.pocket_x,
                                      q.pocket_onehot, s);
        if (gv && from_prior) cmdgen_launch_inpaint_prep(lay, d, c, ip, gv->phar_x, gv->phar_onehot, gv->fix_x, gv->fix_h, q.pocket_x, s);
    }
    if (gu || se) cmdgen_launch_restrain_prep(lay, d, rb, q.pocket_x, s);     // (with groups: of every member; the guidance reads the first member's)
    // One denoising step = the posterior update fused with pass 1 of the next radius graph (the corner's step launch), then the evaluation
    // at the new state: pass 2 of the graph (k_edge_write), k_embed, the L blocks, k_readout.  The chain is: evaluation 0, n_steps x (step +
    // evaluation), decode.
    // The plain and the restrained chain run their evaluations without k_readout where the plan says so (LaunchPlan::readout_in_coord): its
    // feature part rides in the last coordinate launch, the step kernel (it has both forms) makes the velocity and the NaN flag it consumes
    // itself, and k_vel_flag does so once in front of the decode.  Every other kind's evaluations run their own k_readout.
    const bool plain_evals = !gr && !gv && !se;
    int own_vel = 0;
    if (plain_evals) {
        ch.a.plain_chain = 1;
        own_vel = readout_mode(ch.a, c.state, nullptr, nullptr, nullptr);     // (what the evaluations below are launched with)
    }
    ch.start(true);                                  // evaluation 0 (t = 1, or start / timesteps)
    // (a step kernel that leaves X0 / ACC to an evaluation that does not take them over would leave stale positions without any error)
    // (evaluation 0 is already queued when this returns: the chain is abandoned half issued, the handle stays usable - the next chain of any
    // kind starts again from its init launch and k_edge_count, which rewrite everything this one left behind)
    if (plain_evals && ch.a.readout_used != own_vel)
        return fail(h, CMDGEN_ESTATE, "the evaluation and the step kernel disagree on readout_in_coord (%d, %d)", ch.a.readout_used, own_vel);
    // ---- the steps: the one launcher of the corner (the adapters build no other)
    const int corner = (se ? 8 : 0) | (gr ? 4 : 0) | (gv ? 2 : 0) | (gu ? 1 : 0);
    rc = ch.steps({q.noise, q.z_steps_out, q.pocket_steps_out, op_side, op_side2}, n_steps, [&](hipStream_t ss) {
        switch (corner) {
        case 0: cmdgen_launch_step_count(lay, d, c, w, eps, own_vel, ss); break;
        case 1: cmdgen_launch_restrained_step_count(lay, d, c, rb, w, eps, own_vel, ss); break;
        case 2: cmdgen_launch_inpaint_step_count(lay, d, c, ip, w, eps, ss); break;
        case 3: cmdgen_launch_restrained_edit_step_count(lay, d, c, ip, rb, w, eps, ss); break;
        case 4: cmdgen_launch_multi_step_count(lay, d, c, gt, w, eps, ss); break;
        case 5: cmdgen_launch_multi_restrained_step(lay, d, c, gt, rb, w, eps, gd, ss); break;
        case 6: cmdgen_launch_multi_edit_step_count(lay, d, c, gt, ip, w, eps, ss); break;
        case 7: cmdgen_launch_multi_restrained_edit_step(lay, d, c, gt, ip, rb, w, eps, gd, ss); break;
        case 8: cmdgen_launch_diverse_step(lay, d, c, db, w, eps, ss); break;
        case 9: cmdgen_launch_diverse_restrained_step(lay, d, c, rb, db, w, eps, ss); break;
        }
    });
    if (rc) return rc;
    // ---- final p(x, h | z0): the last evaluation above ran at t = 0 (the decode row's w); decode, then the steering part's report on the output
    if (own_vel) cmdgen_launch_vel_flag(ch.a, eps, s);
    if (gr) {
        cmdgen_launch_multi_final(lay, d, decode_buf(c, decode_skip, (size_t)gt.Nu, P), gt, w, eps, q.xh_phar_out, q.xh_pocket_out, ch.k->cog, s);
        if (gu) cmdgen_launch_multi_restrain_energy(lay, d, gt, rb, q.xh_phar_out, q.xh_pocket_out, gu->energy_out, s);
    } else {
        cmdgen_launch_chain_final(lay, d, decode_buf(c, decode_skip, (size_t)lay.Nl, P), w, eps, q.xh_phar_out, q.xh_pocket_out, ch.k->cog, s);
        if (gu) cmdgen_launch_restrain_energy(lay, d, rb, q.xh_phar_out, q.xh_pocket_out, gu->energy_out, s);
    }
    if (se) cmdgen_launch_diverse_overlap(lay, d, db, q.xh_phar_out, q.xh_pocket_out, se->overlap_out, s);
    return ch.close();
}

// the ten entries (and the inpainting alias): each packs what it received
extern "C" int cmdgen_sample_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                   int32_t timesteps, const float* noise, uint64_t seed,
                                   const int64_t* pocket_ids_host, float* xh_phar_out, float* xh_pocket_out,
                                   float* z_steps_out, float* pocket_steps_out, int32_t use_graph, cmdgen_stream stream) {
    return sampling_chain(h, {CHAIN_PLAIN, nullptr, "", CMDGEN_ESTATE, pocket_x, pocket_onehot, timesteps, noise, 0, seed, pocket_ids_host, xh_phar_out,
                              xh_pocket_out, z_steps_out, pocket_steps_out, use_graph, stream, nullptr, nullptr, nullptr, nullptr});
}

extern "C" int cmdgen_restrained_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot, int32_t timesteps,
                                       const cmdgen_restraint* restraints_host, int64_t n_restraints,
                                       float clash_radius, float clash_k, float scale, float max_shift, float guide_below,
                                       const float* noise, uint64_t seed, const int64_t* pocket_ids_host,
                                       float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                       float* energy_out, float* op_energy_out, int32_t use_graph, cmdgen_stream stream) {
    const GuidePart guide{restraints_host, n_restraints, {clash_radius, clash_k, scale, max_shift, guide_below}, energy_out, op_energy_out};
    return sampling_chain(h, {CHAIN_RESTRAINED, "the restrained chain", kGuideFrame, CMDGEN_EINVAL, pocket_x, pocket_onehot, timesteps, noise, 0, seed,
                              pocket_ids_host, xh_phar_out, xh_pocket_out, z_steps_out, pocket_steps_out, use_graph, stream, nullptr, nullptr, &guide,
                              nullptr});
}

extern "C" int cmdgen_diverse_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot, int32_t timesteps,
                                    int64_t n_sets, const int64_t* set_size_host,
                                    float strength, float width, float max_shift, float guide_below,
                                    const float* noise, uint64_t seed, const int64_t* pocket_ids_host,
                                    float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                    float* overlap_out, float* op_overlap_out, int32_t use_graph, cmdgen_stream stream) {
    const SetsPart sets{n_sets, set_size_host, strength, width, max_shift, guide_below, overlap_out, op_overlap_out};
    return sampling_chain(h, {CHAIN_DIVERSE, "the diverse chain", kGuideFrame, CMDGEN_EINVAL, pocket_x, pocket_onehot, timesteps, noise, 0, seed,
                              pocket_ids_host, xh_phar_out, xh_pocket_out, z_steps_out, pocket_steps_out, use_graph, stream, nullptr, nullptr, nullptr,
                              &sets});
}

extern "C" int cmdgen_diverse_restrained_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot, int32_t timesteps,
                                               const cmdgen_restraint* restraints_host, int64_t n_restraints,
                                               float clash_radius, float clash_k, float scale, float max_shift, float guide_below,
                                               int64_t n_sets, const int64_t* set_size_host,
                                               float strength, float width, float diverse_max_shift, float diverse_guide_below,
                                               const float* noise, uint64_t seed, const int64_t* pocket_ids_host,
                                               float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                               float* energy_out, float* op_energy_out, float* overlap_out, float* op_overlap_out,
                                               int32_t use_graph, cmdgen_stream stream) {
    const GuidePart guide{restraints_host, n_restraints, {clash_radius, clash_k, scale, max_shift, guide_below}, energy_out, op_energy_out};
    const SetsPart sets{n_sets, set_size_host, strength, width, diverse_max_shift, diverse_guide_below, overlap_out, op_overlap_out};
    return sampling_chain(h, {CHAIN_DIVERSE_RESTRAINED, "the restrained diverse chain", kGuideFrame, CMDGEN_EINVAL, pocket_x, pocket_onehot, timesteps,
                              noise, 0, seed, pocket_ids_host, xh_phar_out, xh_pocket_out, z_steps_out, pocket_steps_out, use_graph, stream, nullptr,
                              nullptr, &guide, &sets});
}

extern "C" int cmdgen_multi_pocket_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                         int64_t n_groups, const int64_t* group_size_host, const float* weight_host,
                                         int32_t timesteps, const float* noise, uint64_t seed, const int64_t* group_ids_host,
                                         float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                         int32_t use_graph, cmdgen_stream stream) {
    const GroupsPart groups{n_groups, group_size_host, weight_host};
    return sampling_chain(h, {CHAIN_MULTI, "the multi-pocket chain", "", CMDGEN_ESTATE, pocket_x, pocket_onehot, timesteps, noise, 0, seed,
                              group_ids_host, xh_phar_out, xh_pocket_out, z_steps_out, pocket_steps_out, use_graph, stream, &groups, nullptr, nullptr,
                              nullptr});
}

extern "C" int cmdgen_multi_restrained_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                             int64_t n_groups, const int64_t* group_size_host, const float* weight_host, int32_t timesteps,
                                             const cmdgen_restraint* restraints_host, int64_t n_restraints,
                                             float clash_radius, float clash_k, float scale, float max_shift, float guide_below,
                                             const float* noise, uint64_t seed, const int64_t* group_ids_host,
                                             float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                             float* energy_out, float* op_energy_out, int32_t use_graph, cmdgen_stream stream) {
    const GroupsPart groups{n_groups, group_size_host, weight_host};
    const GuidePart guide{restraints_host, n_restraints, {clash_radius, clash_k, scale, max_shift, guide_below}, energy_out, op_energy_out};
    return sampling_chain(h, {CHAIN_MULTI_RESTRAINED, "the restrained multi-pocket chain", kGuideFrame, CMDGEN_ESTATE, pocket_x, pocket_onehot, timesteps,
                              noise, 0, seed, group_ids_host, xh_phar_out, xh_pocket_out, z_steps_out, pocket_steps_out, use_graph, stream, &groups,
                              nullptr, &guide, nullptr});
}

extern "C" int cmdgen_edit_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                 const float* phar_x, const float* phar_onehot, const float* fix_x, const float* fix_h,
                                 int32_t timesteps, int32_t start, int32_t resamplings, int32_t jump_length,
                                 const float* noise, int64_t n_draws, uint64_t seed, const int64_t* pocket_ids_host,
                                 float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                 int32_t use_graph, cmdgen_stream stream) {
    const GivenPart given{phar_x, phar_onehot, fix_x, fix_h, start, resamplings, jump_length};
    return sampling_chain(h, {CHAIN_INPAINT, nullptr, "", CMDGEN_ESTATE, pocket_x, pocket_onehot, timesteps, noise, n_draws, seed, pocket_ids_host,
                              xh_phar_out, xh_pocket_out, z_steps_out, pocket_steps_out, use_graph, stream, nullptr, &given, nullptr, nullptr});
}

extern "C" int cmdgen_inpaint_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                    const float* phar_x, const float* phar_onehot, const float* phar_fixed,
                                    int32_t timesteps, int32_t resamplings, int32_t jump_length,
                                    const float* noise, int64_t n_draws, uint64_t seed, const int64_t* pocket_ids_host,
                                    float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                    int32_t use_graph, cmdgen_stream stream) {
    return cmdgen_edit_chain(h, pocket_x, pocket_onehot, phar_x, phar_onehot, phar_fixed, phar_fixed, timesteps, timesteps, resamplings,
                             jump_length, noise, n_draws, seed, pocket_ids_host, xh_phar_out, xh_pocket_out, z_steps_out,
                             pocket_steps_out, use_graph, stream);
}

extern "C" int cmdgen_restrained_edit_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                            const float* phar_x, const float* phar_onehot, const float* fix_x, const float* fix_h,
                                            int32_t timesteps, int32_t start, int32_t resamplings, int32_t jump_length,
                                            const float* noise, int64_t n_draws, uint64_t seed, const int64_t* pocket_ids_host,
                                            float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                            const cmdgen_restraint* restraints_host, int64_t n_restraints,
                                            float clash_radius, float clash_k, float scale, float max_shift, float guide_below,
                                            float* energy_out, float* op_energy_out, int32_t use_graph, cmdgen_stream stream) {
    const GivenPart given{phar_x, phar_onehot, fix_x, fix_h, start, resamplings, jump_length};
    const GuidePart guide{restraints_host, n_restraints, {clash_radius, clash_k, scale, max_shift, guide_below}, energy_out, op_energy_out};
    return sampling_chain(h, {CHAIN_RESTRAINED_EDIT, "the restrained edit chain", kEditGuideFrame, CMDGEN_ESTATE, pocket_x, pocket_onehot, timesteps, noise,
                              n_draws, seed, pocket_ids_host, xh_phar_out, xh_pocket_out, z_steps_out, pocket_steps_out, use_graph, stream, nullptr,
                              &given, &guide, nullptr});
}

extern "C" int cmdgen_multi_edit_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                       int64_t n_groups, const int64_t* group_size_host, const float* weight_host,
                                       const float* phar_x, const float* phar_onehot, const float* fix_x, const float* fix_h,
                                       int32_t timesteps, int32_t start, int32_t resamplings, int32_t jump_length,
                                       const float* noise, int64_t n_draws, uint64_t seed, const int64_t* group_ids_host,
                                       float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                       int32_t use_graph, cmdgen_stream stream) {
    const GroupsPart groups{n_groups, group_size_host, weight_host};
    const GivenPart given{phar_x, phar_onehot, fix_x, fix_h, start, resamplings, jump_length};
    return sampling_chain(h, {CHAIN_MULTI_EDIT, "the multi-pocket edit chain", "", CMDGEN_ESTATE, pocket_x, pocket_onehot, timesteps, noise, n_draws, seed,
                              group_ids_host, xh_phar_out, xh_pocket_out, z_steps_out, pocket_steps_out, use_graph, stream, &groups, &given, nullptr,
                              nullptr});
}

extern "C" int cmdgen_multi_restrained_edit_chain(cmdgen_handle* h, const float* pocket_x, const float* pocket_onehot,
                                                  int64_t n_groups, const int64_t* group_size_host, const float* weight_host,
                                                  const float* phar_x, const float* phar_onehot, const float* fix_x, const float* fix_h,
                                                  int32_t timesteps, int32_t start, int32_t resamplings, int32_t jump_length,
                                                  const float* noise, int64_t n_draws, uint64_t seed, const int64_t* group_ids_host,
                                                  float* xh_phar_out, float* xh_pocket_out, float* z_steps_out, float* pocket_steps_out,
                                                  const cmdgen_restraint* restraints_host, int64_t n_restraints,
                                                  float clash_radius, float clash_k, float scale, float max_shift, float guide_below,
                                                  float* energy_out, float* op_energy_out, int32_t use_graph, cmdgen_stream stream) {
    const GroupsPart groups{n_groups, group_size_host, weight_host};
    const GivenPart given{phar_x, phar_onehot, fix_x, fix_h, start, resamplings, jump_length};
    const GuidePart guide{restraints_host, n_restraints, {clash_radius, clash_k, scale, max_shift, guide_below}, energy_out, op_energy_out};
    return sampling_chain(h, {CHAIN_MULTI_RESTRAINED_EDIT, "the restrained multi-pocket edit chain", kEditGuideFrame, CMDGEN_ESTATE, pocket_x, pocket_onehot,
                              timesteps, noise, n_draws, seed, group_ids_host, xh_phar_out, xh_pocket_out, z_steps_out, pocket_steps_out, use_graph, stream,
                              &groups, &given, &guide, nullptr});
}

// ---------------------------------------------------------------------------------
// scoring: ConditionalDDPM.score (kernels_score.hip; the level semantics and the output columns are in include/cmdgen_hip.h)
// ---------------------------------------------------------------------------------
// what cmdgen_score_chain and cmdgen_multi_score_chain check of a level list alike, and its rows: one per level
// (alpha_t, sigma_t, t == 0, t / T), then (alpha_T, sigma_T, 0, 1) for the prior KL sums; alpha and sigma are the caller's when it
// supplies them (its own fp32 evaluation of the schedule, as cmdgen_set_step_table)
static int build_level_rows(cmdgen_handle* h, int32_t n_levels, const int32_t* t_levels_host, const float* level_coef_host,
                            std::vector<float>& tables) {
    if (n_levels < 1) return fail(h, CMDGEN_EINVAL, "n_levels=%d must be >= 1", n_levels);
    const int T = h->cfg.timesteps;
    for (int i = 0; i < n_levels; ++i)
        if (t_levels_host[i] < 0 || t_levels_host[i] > T)
            return fail(h, CMDGEN_EINVAL, "level %d is t=%d: levels must be in [0, %d]", i, t_levels_host[i], T);
    if (cmdgen_score_step_lds(h->lay, h->dims) > 64 * 1024)
        return fail(h, CMDGEN_EINVAL, "a sample has %d nodes: the scoring step keeps a sample's positions, z and row sums in LDS (64 KiB)", h->lay.max_n);
    tables.assign((size_t)(n_levels + 1) * 4, 0.f);
    for (int i = 0; i <= n_levels; ++i) {
        const int t = i < n_levels ? t_levels_host[i] : T;
        const float g = h->gamma[(size_t)t];
        tables[4 * i + 0] = level_coef_host ? level_coef_host[2 * i] : sqrtf(sigmoid_h(-g));
        tables[4 * i + 1] = level_coef_host ? level_coef_host[2 * i + 1] : sqrtf(sigmoid_h(g));
        tables[4 * i + 2] = (i < n_levels && t == 0) ? 1.f : 0.f;
        tables[4 * i + 3] = (float)t / (float)T;
    }
    return 0;
}

// the two scoring chains: what an entry received (groups: ConditionalDDPM.score_given_pockets, the definition is in include/cmdgen_hip.h -
// the level rows are the same, the group tables the multi-pocket chain's, behind them in the slot's table block), and their one body
struct ScoringCall {
    ChainKind kind;
    const float *phar_x, *phar_onehot, *pocket_x, *pocket_onehot;
    int32_t n_levels; const int32_t* t_levels_host; const float* level_coef_host;
    const float* noise; uint64_t seed; const int64_t* ids_host;          // ids: of the pockets, or with groups of the groups
    float *terms_out, *member_terms_out, *kl_sums_out;                  // terms: per level and sample, or with groups per level and group (then member_terms: per member, or null)
    int32_t use_graph; cmdgen_stream stream;
    const GroupsPart* groups;
};
static int scoring_chain(cmdgen_handle* h, const ScoringCall& q) {
    const GroupsPart* const gr = q.groups;
    int rc = check_ready(h); if (rc) return rc;
    rc = refuse_joint_no_com(h, "scoring", kOwnPocketTerms); if (rc) return rc;
    bool missing = !q.phar_x || !q.phar_onehot || !q.pocket_x || !q.pocket_onehot || !q.t_levels_host || !q.terms_out || !q.kl_sums_out;
    if (gr) missing |= !gr->size_host || !gr->weight_host;
    if (missing) return fail(h, CMDGEN_EINVAL, "null pointer");
    TableBlock tables;
    rc = build_level_rows(h, q.n_levels, q.t_levels_host, q.level_coef_host, tables.f); if (rc) return rc;
    const float alpha_T = tables.f[4 * (size_t)q.n_levels];
    GroupPlan gp;
    if (gr) {
        rc = build_group_plan(h, gr->n, gr->size_host, gr->weight_host, q.ids_host, gp); if (rc) return rc;
        append_group_tables(tables, gp, gr->weight_host, h->lay.B);
    }
    Chain ch;
    rc = ch.open(h, q.kind, tables, q.n_levels, alloc_scoring, gr ? gp.gid.data() : q.ids_host, q.noise, q.seed, nullptr, nullptr, q.use_graph, q.stream);
    if (rc) return rc;
    const Layout& lay = h->lay; const Dims& d = h->dims; const Work& w = h->work;
    const ChainBuf& c = ch.c;
    ScoreBuf sc = ch.k->score;
    sc.out = q.terms_out;
    const GroupTab gt = group_tab(*ch.k, gp);
    if (gr) cmdgen_launch_multi_score_init(lay, d, c, sc, gt, alpha_T, q.phar_x, q.phar_onehot, q.pocket_x, q.pocket_onehot, q.kl_sums_out, ch.s);
    else cmdgen_launch_score_init(lay, d, c, sc, alpha_T, q.phar_x, q.phar_onehot, q.pocket_x, q.pocket_onehot, q.kl_sums_out, ch.s);
    ch.start(false);                                 // every evaluation follows a step launch
    // the level rows, the group tables and the clean rows are slot buffers (a changed level list, grouping or weight prepares the slot again
    // and drops its graph); the captured steps read the caller's draws and write its outputs
    rc = ch.steps({q.noise, q.terms_out, q.member_terms_out, nullptr, nullptr}, q.n_levels, [&](hipStream_t ss) {
        if (gr) cmdgen_launch_multi_score_step(lay, d, c, sc, gt, w, w.eps_tmp, q.member_terms_out, ss);
        else cmdgen_launch_score_step(lay, d, c, sc, w, w.eps_tmp, ss);
    });
    if (rc) return rc;
    if (gr) cmdgen_launch_multi_score_final(lay, d, c, sc, gt, w, w.eps_tmp, q.member_terms_out, ch.s);
    else cmdgen_launch_score_final(lay, d, c, sc, w, w.eps_tmp, ch.s);
    return ch.close();
}

extern "C" int cmdgen_score_chain(cmdgen_handle* h, const float* phar_x, const float* phar_onehot,
                                  const float* pocket_x, const float* pocket_onehot,
                                  int32_t n_levels, const int32_t* t_levels_host, const float* level_coef_host,
                                  const float* noise, uint64_t seed, const int64_t* pocket_ids_host,
                                  float* level_terms_out, float* kl_sums_out, int32_t use_graph, cmdgen_stream stream) {
    return scoring_chain(h, {CHAIN_SCORE, phar_x, phar_onehot, pocket_x, pocket_onehot, n_levels, t_levels_host, level_coef_host, noise, seed,
                             pocket_ids_host, level_terms_out, nullptr, kl_sums_out, use_graph, stream, nullptr});
}

extern "C" int cmdgen_multi_score_chain(cmdgen_handle* h, const float* phar_x, const float* phar_onehot,
                                        const float* pocket_x, const float* pocket_onehot,
                                        int64_t n_groups, const int64_t* group_size_host, const float* weight_host,
                                        int32_t n_levels, const int32_t* t_levels_host, const float* level_coef_host,
                                        const float* noise, uint64_t seed, const int64_t* group_ids_host,
                                        float* group_terms_out, float* member_terms_out, float* kl_sums_out,
                                        int32_t use_graph, cmdgen_stream stream) {
    const GroupsPart groups{n_groups, group_size_host, weight_host};
    return scoring_chain(h, {CHAIN_MULTI_SCORE, phar_x, phar_onehot, pocket_x, pocket_onehot, n_levels, t_levels_host, level_coef_host, noise, seed,
                             group_ids_host, group_terms_out, member_terms_out, kl_sums_out, use_graph, stream, &groups});
}

extern "C" int cmdgen_chain_status(cmdgen_handle* h, float* max_rel, float* max_cog, int64_t* nan_resets, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    const ChainSlot& k = h->chains[h->last_chain];
    const int K = k.n_steps;
    if (K < 0) return fail(h, CMDGEN_ESTATE, "no chain has run");
    hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    std::vector<unsigned int> chk((size_t)(K + 3) * 2);
    HIPCHK(h, hipMemcpy(chk.data(), k.check, chk.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
    float worst = 0.f;
    for (int i = 0; i < K + 2 && worst == worst; ++i) {
        float largest, err;
        memcpy(&largest, &chk[2 * i], 4); memcpy(&err, &chk[2 * i + 1], 4);
        const float rel = err / (largest + 1e-10f);
        if (rel > worst || rel != rel) worst = rel;      // a NaN sticks: the reference's `assert rel_error < 1e-2` fails on it
    }
    if (max_rel) *max_rel = worst;
    unsigned int cog; HIPCHK(h, hipMemcpy(&cog, k.cog, 4, hipMemcpyDeviceToHost));
    if (max_cog) memcpy(max_cog, &cog, 4);
    unsigned long long cnt[8];
    HIPCHK(h, hipMemcpy(cnt, h->work.counters, sizeof cnt, hipMemcpyDeviceToHost));
    if (nan_resets) *nan_resets = (int64_t)cnt[4];
    return CMDGEN_OK;
}

// ---------------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------------
extern "C" int cmdgen_get_counters(cmdgen_handle* h, cmdgen_counters* out, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    unsigned long long cnt[8];
    HIPCHK(h, hipMemcpy(cnt, h->work.counters, sizeof cnt, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->evaluations = cnt[0]; out->edges = cnt[1]; out->edges_phar = cnt[2]; out->nodes = cnt[3]; out->nan_resets = cnt[4];
    out->edges_skipped = cnt[6]; out->node_rows_skipped = cnt[7]; out->half_low_range = cnt[HALF_LOW_SLOT];
    return CMDGEN_OK;
}

extern "C" int cmdgen_reset_counters(cmdgen_handle* h, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    hipSetDevice(h->device);
    HIPCHK(h, hipMemsetAsync(h->work.counters, 0, 8 * sizeof(unsigned long long), (hipStream_t)stream));
    return CMDGEN_OK;
}

extern "C" int cmdgen_profile_evaluation(cmdgen_handle* h, const float* xh_phar, const float* xh_pocket, const float* t,
                                         float* eps_phar, cmdgen_kernel_times* out, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (!out) return fail(h, CMDGEN_EINVAL, "null output");
    if (h->dims.joint) return fail(h, CMDGEN_ESTATE, "cmdgen_profile_evaluation supports the conditional model only");
    if (h->dims.S != 1) return fail(h, CMDGEN_ESTATE, "cmdgen_profile_evaluation supports inv_sublayers = 1 only (cmdgen_set_kernel_profiling works for any)");
    hipStream_t s = (hipStream_t)stream;
    rc = begin_work(h, s); if (rc) return rc;
    const int L = h->dims.L;
    const int nev = 2 * (3 + 3 * L);
    std::vector<hipEvent_t> ev(nev);
    for (auto& e : ev) HIPCHK(h, hipEventCreate(&e));
    EvalLaunch a = make_launch(h);
    ++h->eval_gen;
    cmdgen_launch_eval(a, xh_phar, xh_pocket, t, nullptr, nullptr, eps_phar, nullptr, s, ev.data());
    cmdgen_launch_nan_fix(a, eps_phar, s);
    HIPCHK(h, hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    auto ms = [&](int i) { float m = 0.f; hipEventElapsedTime(&m, ev[2 * i], ev[2 * i + 1]); return m; };
    int i = 0;
    out->edge_build_ms = ms(i++); out->embed_ms = ms(i++);
    for (int l = 0; l < L; ++l) {
        out->edge_msg_ms += ms(i++); out->node_ms += ms(i++); out->edge_coord_ms += ms(i++);
    }
    out->readout_ms = ms(i++);
    out->edge_msg_launches = L; out->node_launches = L; out->edge_coord_launches = L;
    for (auto& e : ev) hipEventDestroy(e);
    return CMDGEN_OK;
}

extern "C" int cmdgen_set_gemm_mode(cmdgen_handle* h, int32_t split_bf16) {
    if (!h) return CMDGEN_EINVAL;
    if (split_bf16 && h->dims.sin) return fail(h, CMDGEN_ESTATE, "sin_embedding runs on the fp32 matrix instruction only (the split engine's tile builders carry two scalar edge features)");
    if (h->gemm_split != (split_bf16 != 0)) {
        drop_graphs(h);                 // captured graphs bake the kernel choice in; the pocket cache is rebuilt per chain anyway
        h->gemm_split = split_bf16 != 0;
        if (h->have_layout) replan(h);
    }
    return CMDGEN_OK;
}

extern "C" int cmdgen_query(cmdgen_handle* h, const char* key, int64_t* value) {
    if (!h || !key || !value) return CMDGEN_EINVAL;
    if (!h->have_layout) return fail(h, CMDGEN_ESTATE, "no batch layout (cmdgen_set_layout)");
    const std::string k = key;
    if (plan_query(h->plan, key, value)) return CMDGEN_OK;      // the launch keys: what the planner resolved (1 = the fp32 matrix instruction, 6 = three bf16
                                                                // pieces per operand, 3 = the half engine, for the *_mfmas_per_product keys)
    if (k == "eval_gen") *value = h->eval_gen;
    else if (k == "chain_graphs") { int64_t n = 0; for (const ChainSlot& c : h->chains) n += c.graph != nullptr ? 1 : 0; *value = n; }   // captured step graphs held
    else if (k == "train_half_ran") *value = h->train_fwd_half;
    else if (k == "train_range_event") *value = h->h_norm && !h->norm_pending ? (int64_t)h->h_norm[1] : 0;     // of the last collected norm
    else if (k == "train_edges") *value = h->train_E;
    else if (k == "train_coord_edges") *value = h->train_Ec;
    else return fail(h, CMDGEN_EINVAL, "unknown query '%s'", key);
    return CMDGEN_OK;
}

extern "C" int cmdgen_time_evaluation(cmdgen_handle* h, const float* xh_phar, const float* xh_pocket, const float* t,
                                      float* eps_phar, int32_t graph_len, int32_t replays, float* mean_ms, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (!xh_phar || !xh_pocket || !t || !eps_phar || !mean_ms || graph_len < 1 || replays < 1) return fail(h, CMDGEN_EINVAL, "bad arguments");
    if (h->dims.joint) return fail(h, CMDGEN_ESTATE, "cmdgen_time_evaluation supports the conditional model only");
    hipStream_t caller = (hipStream_t)stream, s = caller;
    if (caller == nullptr) {                             // the legacy default stream cannot be captured
        rc = own_stream(h); if (rc) return rc;
        HIPCHK(h, hipDeviceSynchronize());
        s = h->own_stream;
    }
    rc = begin_work(h, s); if (rc) return rc;
    EvalLaunch a = make_launch(h);
    ++h->eval_gen;
    hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // every exit below releases what it holds: a failure between Begin- and EndCapture must still end the capture (the
    // caller's stream would otherwise stay in capture mode and poison every later launch on it)
    hipError_t err = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (err != hipSuccess) return fail(h, CMDGEN_EHIP, "hipStreamBeginCapture: %s", hipGetErrorString(err));
    for (int i = 0; i < graph_len; ++i) {
        cmdgen_launch_eval(a, xh_phar, xh_pocket, t, nullptr, nullptr, eps_phar, nullptr, s, nullptr);
        cmdgen_launch_nan_fix(a, eps_phar, s);
    }
    const hipError_t launch_err = hipGetLastError();
    err = hipStreamEndCapture(s, &g);                    // always: also after a failed launch
    if (err == hipSuccess && launch_err != hipSuccess) err = launch_err;
    if (err == hipSuccess) err = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    if (g) hipGraphDestroy(g);
    if (err == hipSuccess) err = hipEventCreate(&e0);
    if (err == hipSuccess) err = hipEventCreate(&e1);
    if (err == hipSuccess) err = hipGraphLaunch(ge, s);  // warm
    if (err == hipSuccess) err = hipEventRecord(e0, s);
    for (int i = 0; i < replays && err == hipSuccess; ++i) err = hipGraphLaunch(ge, s);
    if (err == hipSuccess) err = hipEventRecord(e1, s);
    if (err == hipSuccess) err = hipEventSynchronize(e1);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (ge) hipGraphExecDestroy(ge);
    if (err != hipSuccess) return fail(h, CMDGEN_EHIP, "cmdgen_time_evaluation: %s", hipGetErrorString(err));
    *mean_ms = ms / ((float)replays * (float)graph_len);
    return CMDGEN_OK;
}

extern "C" int cmdgen_time_edge_kernel(cmdgen_handle* h, int32_t layer, int32_t reps, float* mean_ms, cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (layer < 0 || (layer & 0xff) >= h->dims.L || reps < 1 || !mean_ms) return fail(h, CMDGEN_EINVAL, "bad arguments");
    hipSetDevice(h->device);
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0)); HIPCHK(h, hipEventCreate(&e1));
    EvalLaunch a = make_launch(h);
    ++h->eval_gen;
    a.ablate = (layer >> 8) & 0xff;                                 // bits 8.. of `layer`: phase-ablation mask (timing only)
    layer &= 0xff;
    cmdgen_launch_edge_msg_only(a, layer, s);                       // warm
    HIPCHK(h, hipEventRecord(e0, s));
    for (int i = 0; i < reps; ++i) cmdgen_launch_edge_msg_only(a, layer, s);
    HIPCHK(h, hipEventRecord(e1, s));
    HIPCHK(h, hipEventSynchronize(e1));
    float ms = 0.f; hipEventElapsedTime(&ms, e0, e1);
    *mean_ms = ms / (float)reps;
    // the replays accumulated into agg; restore the invariant "agg is zero between blocks"
    HIPCHK(h, hipMemsetAsync(h->work.agg, 0, (size_t)h->lay.N * h->dims.H * sizeof(float), s));
    hipEventDestroy(e0); hipEventDestroy(e1);
    return CMDGEN_OK;
}

extern "C" int cmdgen_debug_stamps(cmdgen_handle* h, uint64_t* out64, int32_t reset) {
    if (!h || !h->have_layout || !out64) return CMDGEN_EINVAL;
    hipSetDevice(h->device);
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(out64, h->work.dbg, 64 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(h, hipMemset(h->work.dbg, 0, 64 * sizeof(uint64_t)));
    return CMDGEN_OK;
}

extern "C" int cmdgen_set_kernel_profiling(cmdgen_handle* h, int32_t on) {
    if (!h) return CMDGEN_EINVAL;
    h->kernel_profiling = on != 0;
    return CMDGEN_OK;
}

extern "C" int cmdgen_get_kernel_profile(cmdgen_handle* h, float total_ms[3], int64_t launches[3], cmdgen_stream stream) {
    int rc = check_ready(h); if (rc) return rc;
    hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    if (h->own_stream) HIPCHK(h, hipStreamSynchronize(h->own_stream));
    for (int k = 0; k < 3; ++k) {
        std::vector<hipEvent_t>& ev = h->prof_events[k];
        double tot = 0.0;
        const size_t n = ev.size() / 2;
        for (size_t i = 0; i < n; ++i) {
            float ms = 0.f;
            HIPCHK(h, hipEventSynchronize(ev[2 * i + 1]));
            hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]);
            tot += ms;
        }
        for (hipEvent_t e : ev) hipEventDestroy(e);
        ev.clear();
        if (total_ms) total_ms[k] = (float)tot;
        if (launches) launches[k] = (int64_t)n;
    }
    return CMDGEN_OK;
}

extern "C" int cmdgen_debug_noise(cmdgen_handle* h, uint64_t seed, int64_t pocket_id, int32_t draw, int32_t n_nodes,
                                  int32_t width, float* out_dev, cmdgen_stream stream) {
    if (!h || !out_dev || n_nodes < 1 || width < 1 || width > 16) return fail(h, CMDGEN_EINVAL, "bad arguments");
    hipSetDevice(h->device);
    cmdgen_launch_debug_noise(seed, pocket_id, draw, n_nodes, width, out_dev, (hipStream_t)stream);
    HIPCHK(h, hipGetLastError());
    return CMDGEN_OK;
}
