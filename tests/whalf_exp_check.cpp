// Host check of the half engine's scale rule (cmdgen_amd/csrc/cmdgen_wlayout.h, whalf_exp): it must give the exponent that BOTH
// rules it replaced gave - the host packer's frexp rule and the device re-packer's exponent-bit rule - for every largest weight in
// (0, 3.0e38): every exponent field, subnormals included, with the smallest, the largest and some middle mantissas.  Above 3.0e38
// the rule gives 0 (the former device rule; the packs overflow fp16 there under any scale).  Built and run by tests/test_host_cpu.py.
#include "cmdgen_wlayout.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>

static int host_rule(float mx) {        // cmdgen_api.hip, pack_half, before the rules were merged
    int e = 0;
    if (mx > 0.f && std::isfinite(mx)) { int ex; std::frexp(mx, &ex); e = 12 - ex; }
    return std::max(-40, std::min(40, e));
}
static int device_rule(float mx) {      // kernels_train_repack.hip, k_repack_half / k_wmax16, before the rules were merged
    uint32_t u; memcpy(&u, &mx, 4);
    int e = 0;
    if (mx > 0.f && mx < 3.0e38f) e = 12 - ((int)((u >> 23) & 0xffu) - 126);
    return std::max(-40, std::min(40, e));
}

int main() {
    const uint32_t mant[] = {0u, 1u, 2u, 0x000400u, 0x2aaaaau, 0x3fffffu, 0x400000u, 0x400001u, 0x555555u, 0x7ffffeu, 0x7fffffu};
    long checked = 0, bad = 0;
    for (uint32_t ex = 0; ex < 255; ++ex)
        for (uint32_t m : mant) {
            const uint32_t u = (ex << 23) | m;
            float mx; memcpy(&mx, &u, 4);
            if (!(mx > 0.f)) continue;
            const int e = whalf_exp(mx);
            if (mx < 3.0e38f) {
                ++checked;
                if (e != host_rule(mx) || e != device_rule(mx)) { printf("mx = %a: %d, host rule %d, device rule %d\n", mx, e, host_rule(mx), device_rule(mx)); ++bad; }
                if (e > -40 && e < 40 && !(mx * whalf_pow2(e) >= 2048.f && mx * whalf_pow2(e) < 4096.f)) { printf("mx = %a: scaled to %a\n", mx, mx * whalf_pow2(e)); ++bad; }
            } else if (e != 0) { printf("mx = %a: %d above the rule's range\n", mx, e); ++bad; }
        }
    for (int e = -40; e <= 40; ++e)
        if (whalf_pow2(e) != std::ldexp(1.0f, e)) { printf("whalf_pow2(%d) = %a\n", e, whalf_pow2(e)); ++bad; }
    if (whalf_exp(0.f) != 0 || whalf_exp(INFINITY) != 0 || whalf_exp(NAN) != 0 || whalf_exp(FLT_MAX) != 0) { printf("a special value does not give 0\n"); ++bad; }
    printf("checked %ld bad %ld\n", checked, bad);
    return bad ? 1 : 0;
}
