// cmdgen_wlayout.h - the MFMA fragment orders of a packed Linear weight (WPack, cmdgen_dev.h), each written once: the host packs
// the sampler's weights with these maps (cmdgen_api.hip), the training step re-packs its parameters on the device with the same
// maps (kernels_train_repack.hip), and the same tile kernels read both.
//
// A weight W[out][in] (nn.Linear layout, in a multiple of KBLK) is cut into n-tiles of ROWS output rows and k-blocks of KBLK
// inputs.  Fragment (nt, kb) is 64 lanes x PER values; lane l holds, of row ROWS nt + l % ROWS, the values k0 + koff(j), j < PER,
// with k0 = KBLK kb + (run of the lane group g = l / ROWS):
//     WFrag<32, 4>   w32          v_mfma_f32_32x32x2_f32             KBLK  8   k =  8 kb + 4 g + j
//     WFrag<16, 4>   w16          v_mfma_f32_16x16x4_f32             KBLK 16   k = 16 kb + 4 g + j
//     WFrag<32, 8>   ws,   wh     v_mfma_f32_32x32x16_bf16 / _f16    KBLK 16   k = 16 kb + 8 g + j
//     WFrag<16, 8>   ws16, wh16   v_mfma_f32_16x16x32_bf16 / _f16    KBLK 32   k = 32 kb + 4 g + j (j < 4), 32 kb + 16 + 4 g + j - 4 (j >= 4)
// A lane's PER values are one 16-byte piece (four floats, eight bf16 or fp16), so one load per lane feeds PER / (values per MFMA)
// k-steps, and the A operand is read from LDS with the same pairing (the fp32 orders: step j pairs lane group g with k0 + j, a fixed
// re-association of the dot product; the 16-row bf16 / fp16 order: the two runs of four are what one A-side read delivers,
// cmdgen_split.h).  An order with PIECES pieces per weight - ws / ws16: three bf16, w = w0 + w1 + w2 up to 2^-24 |w|; wh / wh16: two
// fp16 of w 2^e, whalf_exp - keeps the pieces of a fragment behind one another: wfrag_piece.  The readers (frag_ptr, sfrag_ptr,
// sfrag16_ptr, hfrag_ptr, nw_frag, w_frag, n64_tile) fold this arithmetic into their buffer offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

template <int ROWS_, int PER_> struct WFrag {
    static constexpr int ROWS = ROWS_, PER = PER_, KBLK = PER * (64 / ROWS);
    static constexpr bool TWO_RUNS = ROWS == 16 && PER == 8;
    static __host__ __device__ __forceinline__ int row(int nt, int lane) { return ROWS * nt + (lane & (ROWS - 1)); }
    static __host__ __device__ __forceinline__ int k0(int kb, int lane) { return KBLK * kb + (TWO_RUNS ? 4 : PER) * (lane / ROWS); }
    static __host__ __device__ __forceinline__ int koff(int j) { return TWO_RUNS && j >= 4 ? j + 12 : j; }
};
// 16-byte unit of piece s of fragment `frag` = nt * (in / KBLK) + kb
__host__ __device__ __forceinline__ size_t wfrag_piece(int frag, int pieces, int s, int lane) { return (size_t)(frag * pieces + s) * 64 + lane; }

// The half engine's power-of-two weight scale 2^e: e puts the largest |w| of a matrix, mx, into [2^11, 2^12), so that both fp16
// pieces of every weight that matters are normal numbers; clamped to [-40, 40] (subnormal mx: 40).  The rule reads the exponent bits
// (the device's former rule; it equals the host's former frexp rule for every mx in (0, 3.0e38)): mx = 0, mx >= 3.0e38, infinite or
// NaN give e = 0 - those packs overflow fp16 under any scale.
__host__ __device__ __forceinline__ int whalf_exp(float mx) {
    uint32_t bits;
    __builtin_memcpy(&bits, &mx, 4);
    int e = 0;
    if (mx > 0.f && mx < 3.0e38f) e = 12 - ((int)((bits >> 23) & 0xffu) - 126);     // mx = m 2^ex, m in [0.5, 1): mx 2^e in [2^11, 2^12)
    return max(-40, min(40, e));
}
__host__ __device__ __forceinline__ float whalf_pow2(int e) {     // 2^e, |e| <= 126
    const uint32_t bits = (uint32_t)(127 + e) << 23;
    float p;
    __builtin_memcpy(&p, &bits, 4);
    return p;
}
