// plan_readout_check.cpp - the launch planner (csrc/cmdgen_plan.h) on the host, for tests/test_plan_readout_cpu.py: the launch keys plan_check.cpp
// prints, then readout_in_coord.  Plain C++, no GPU, no HIP header.
//   stdin:  per plan  H L S dyn joint no_cutoff n_cus gemm_split packs training B nph npk n_opts {key value}      (B equal samples)
//           (dyn: joint_nf + condition_time; packs: 1 = what cmdgen_finalize_weights uploads for hidden size H, 0 = none)
//   stdout: per plan one line: the 17 recorded launch keys in plan_check.cpp's order, then readout_in_coord
#include "cmdgen_plan.h"

#include <iostream>
#include <vector>

static const char* const kKeys[] = {"node_mt", "edge_mt", "coord_mt", "edge_grid", "coord_grid", "e128_fused", "gemm_split", "half_engine", "node16_split",
                                    "node64", "node16w", "proj_in_coord", "edge_fullk", "dead_skip", "msg_mfmas_per_product", "node_mfmas_per_product",
                                    "coord_mfmas_per_product", "readout_in_coord"};

int main() {
    PlanInput in;
    int joint, no_cutoff, split, packs, training, n_opts;
    int64_t nph, npk;
    while (std::cin >> in.H >> in.L >> in.S >> in.dyn >> joint >> no_cutoff >> in.n_cus >> split >> packs >> training >> in.B >> nph >> npk >> n_opts) {
        std::map<std::string, int64_t> opts;
        for (int i = 0; i < n_opts; ++i) { std::string k; int64_t v; std::cin >> k >> v; opts[k] = v; }
        if (!std::cin || in.B < 1) { std::cerr << "bad plan line\n"; return 2; }
        const std::vector<int64_t> a(in.B, nph), b(in.B, npk);
        in.joint = joint; in.cutoff = !no_cutoff; in.gemm_split = split; in.training = training; in.embed_pack = packs != 0; in.opts = &opts;
        in.nph = a.data(); in.npk = b.data();
        in.Nl = (int)(in.B * nph); in.N = (int)(in.B * (nph + npk)); in.max_n = (int)(nph + npk);
        in.E = in.N * 9; in.Ec = in.Nl * 15;
        in.W2 = in.W3 = in.W7 = in.Wpq_e = PlanPacks{};
        if (training) { in.W2 = in.W7 = PlanPacks{packs != 0, packs != 0, false, false}; in.W3 = in.Wpq_e = PlanPacks{false, false, false, packs != 0}; }
        else if (packs) { in.W2 = PlanPacks::of_uploaded(in.H); in.W3 = PlanPacks::of_uploaded(2 * in.H); in.W7 = in.W2; in.Wpq_e = in.W2; }
        const LaunchPlan p = make_plan(in);
        for (const char* k : kKeys) { int64_t v = -1; if (!plan_query(p, k, &v)) return 3; std::cout << v << ' '; }
        std::cout << '\n';
    }
    return 0;
}
