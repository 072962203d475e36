// restrained_edit_lds_check.cpp - prints plan_restrained_edit_step_lds, plan_restrained_step_lds and PLAN_RESTRAINED_LDS_MAX (csrc/cmdgen_plan.h) for the
// "max_n P" pairs on stdin, one line each: plain host C++, compiled by test_restrained_edit_cpu.py as tests/plan_check.cpp is.
#include "cmdgen_plan.h"

#include <iostream>

int main() {
    int max_n, P;
    while (std::cin >> max_n >> P)
        std::cout << plan_restrained_edit_step_lds(max_n, P) << ' ' << plan_restrained_step_lds(max_n, P) << ' ' << PLAN_RESTRAINED_LDS_MAX << '\n';
    return 0;
}
