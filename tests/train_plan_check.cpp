// train_plan_check.cpp - the training step's GEMM planners (csrc/cmdgen_train_plan.h) on the host, for tests/test_host_cpu.py: plain C++, no GPU,
// no HIP header.
//   stdin:  tune wgrad_split wgrad_tile wgrad_k128 wgrad_split_wgs128 wgrad_split_wgs64 wgrad_wgs dgrad_mt      (holds until the next tune line)
//           wgrad K bf16 split3 force3 n {M N lddy%4 ldx%4 aligned16 xs}
//           sgemm ta tb M N K a_vec b_vec split_k bf16 epi
//           dgrad M force_mt
//   stdout: per wgrad line  kernel pieces xs grid[3] kchunk zsplit;  per sgemm line  kt grid[3] kchunk z epi slot;  per dgrad line  rows per tile
#include "cmdgen_train_plan.h"

#include <iostream>
#include <string>

int main() {
    std::ios::sync_with_stdio(false);
    TrainTune tune;
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "tune") {
            std::cin >> tune.wgrad_split >> tune.wgrad_tile >> tune.wgrad_k128 >> tune.wgrad_split_wgs128 >> tune.wgrad_split_wgs64 >> tune.wgrad_wgs >> tune.dgrad_mt;
        } else if (cmd == "wgrad") {
            int K, bf16, split3, force3;
            WgradShapes g;
            std::cin >> K >> bf16 >> split3 >> force3 >> g.n;
            if (!std::cin || g.n < 1 || g.n > 8) { std::cerr << "bad wgrad line\n"; return 2; }
            for (int p = 0; p < g.n; ++p) {
                int aligned;
                std::cin >> g.p[p].M >> g.p[p].N >> g.p[p].lddy_mod4 >> g.p[p].ldx_mod4 >> aligned >> g.p[p].xs;
                g.p[p].aligned16 = aligned != 0;
            }
            const WgradPlan p = plan_wgrad(g, K, bf16 != 0, split3 != 0, force3 != 0, tune);
            std::cout << (int)p.kernel << ' ' << p.pieces << ' ' << p.xs << ' ' << p.grid[0] << ' ' << p.grid[1] << ' ' << p.grid[2] << ' ' << p.kchunk << ' '
                      << p.zsplit << '\n';
        } else if (cmd == "sgemm") {
            int ta, tb, M, N, K, av, bv, split_k, bf16, epi;
            std::cin >> ta >> tb >> M >> N >> K >> av >> bv >> split_k >> bf16 >> epi;
            const SgemmPlan p = plan_sgemm(ta != 0, tb != 0, M, N, K, av != 0, bv != 0, split_k, bf16 != 0, epi);
            std::cout << p.kt << ' ' << p.grid[0] << ' ' << p.grid[1] << ' ' << p.grid[2] << ' ' << p.kchunk << ' ' << p.z << ' ' << p.epi << ' ' << p.slot() << '\n';
        } else if (cmd == "dgrad") {
            int M, force_mt;
            std::cin >> M >> force_mt;
            std::cout << plan_dgrad(M, tune, force_mt) << '\n';
        } else { std::cerr << "unknown command " << cmd << '\n'; return 2; }
        if (!std::cin) { std::cerr << "bad " << cmd << " line\n"; return 2; }
    }
    return 0;
}
