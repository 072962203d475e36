// plan_check.cpp - the launch planner (csrc/cmdgen_plan.h) on the host, for tests/test_host_cpu.py: plain C++, no GPU, no HIP header.
//   stdin:  layout B nph[B] npk[B]                                     (layouts are numbered in the order they arrive)
//           plan H L S joint sin no_cutoff n_cus gemm_split packs training E Ec layout n_opts {key value}
//           (packs, sampler: 1 = the packs cmdgen_finalize_weights uploads for hidden size H, 0 = none; training forward: what the step can
//           re-pack, bit 0 = split packs of W2 / W7, bit 1 = their half packs, bit 2 = the 16-row half packs of W3 / Wpq_e)
//   stdout: per plan one line, the launch keys of cmdgen_query in the order of kKeys, then what the launchers switch on and the training
//           step reads: msg node coord (kernel enums) msg_eng node_eng coord_eng e128_grid embed_mt write_embed reads_frag fwd_half node_half
#include "cmdgen_plan.h"

#include <iostream>
#include <vector>

static const char* const kKeys[] = {"node_mt", "edge_mt", "coord_mt", "edge_grid", "coord_grid", "e128_fused", "gemm_split", "half_engine", "node16_split",
                                    "node64", "node16w", "proj_in_coord", "edge_fullk", "dead_skip", "msg_mfmas_per_product", "node_mfmas_per_product",
                                    "coord_mfmas_per_product"};

int main() {
    std::ios::sync_with_stdio(false);
    std::vector<std::vector<int64_t>> nph, npk;
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "layout") {
            int B; std::cin >> B;
            std::vector<int64_t> a(B), b(B);
            for (auto& v : a) std::cin >> v;
            for (auto& v : b) std::cin >> v;
            nph.push_back(a); npk.push_back(b);
        } else if (cmd == "plan") {
            PlanInput in;
            int joint, sin, no_cutoff, split, packs, training, layout, n_opts;
            std::cin >> in.H >> in.L >> in.S >> joint >> sin >> no_cutoff >> in.n_cus >> split >> packs >> training >> in.E >> in.Ec >> layout >> n_opts;
            std::map<std::string, int64_t> opts;
            for (int i = 0; i < n_opts; ++i) { std::string k; int64_t v; std::cin >> k >> v; opts[k] = v; }
            if (!std::cin || layout < 0 || layout >= (int)nph.size()) { std::cerr << "bad plan line\n"; return 2; }
            in.joint = joint; in.sin = sin; in.cutoff = !no_cutoff; in.gemm_split = split; in.training = training; in.opts = &opts;
            in.B = (int)nph[layout].size(); in.nph = nph[layout].data(); in.npk = npk[layout].data();
            for (int b = 0; b < in.B; ++b) {
                const int64_t n = in.nph[b] + in.npk[b];
                in.Nl += (int)in.nph[b]; in.N += (int)n;
                if (n > in.max_n) in.max_n = (int)n;
            }
            if (training) { in.W2 = in.W7 = PlanPacks{(packs & 1) != 0, (packs & 2) != 0, false, false}; in.W3 = in.Wpq_e = PlanPacks{false, false, false, (packs & 4) != 0}; }
            else if (packs) { in.W2 = PlanPacks::of_uploaded(in.H); in.W3 = PlanPacks::of_uploaded(2 * in.H); in.W7 = in.W2; in.Wpq_e = in.W2; }
            const LaunchPlan p = make_plan(in);
            for (const char* k : kKeys) { int64_t v = -1; if (!plan_query(p, k, &v)) return 3; std::cout << v << ' '; }
            std::cout << (int)p.msg << ' ' << (int)p.node << ' ' << (int)p.coord << ' ' << (int)p.msg_eng << ' ' << (int)p.node_eng << ' ' << (int)p.coord_eng << ' '
                      << p.e128_grid << ' ' << p.embed_mt << ' ' << p.write_embed << ' ' << p.reads_frag << ' ' << p.fwd_half << ' ' << p.node_half << '\n';
        } else { std::cerr << "unknown command " << cmd << '\n'; return 2; }
    }
    return 0;
}
