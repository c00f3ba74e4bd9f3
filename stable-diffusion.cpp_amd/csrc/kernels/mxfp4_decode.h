// mxfp4_decode.h — MXFP4 codes -> f16 weights in registers (kernels/bquant.hip; scripts/mxfp4_decode_probe.hip measures both routes below on the device).
//
// block_mxfp4 {u8 e; u8 qs[16]}: y = kvalues[q] * 2^(e - 128), kvalues = {0, 1, 2, 3, 4, 6, 8, 12, and their negatives} (the e2m1 values doubled); the device
// weight is w16 = f16(y), round to nearest even.  y = k * 2^n is exact, so the ONE rounding is into f16: it acts only below 2^-14 (subnormals, ties at k = 3, 6,
// 12) and at overflow.
//
// Integer route (mx4_prep + mx4_w4).  n is split as a + r:
//   a = clamp(n, -14, 12)        k * 2^a is a NORMAL f16 for every k != 0: its bits are f16(k * 2^-14) + ((a + 14) << 10).  Only the high byte of an f16 of k is
//                                non-zero (k has two significant bits), so the eight magnitudes are eight BYTES {00 04 08 0A | 0C 0E 10 12} + 4 (a + 14) (at most
//                                0x7A: no carry between bytes, code 0 stays 0): two registers per block, and ONE v_perm_b32 looks up four codes (selector = code & 7).
//                                Code bit 3 moves to bit 7 of the byte, the sign.  Two more v_perm_b32 put the four bytes above zero low bytes: two packed half2.
//   r = clamp(n - a, -24, 15)    the rest, 0 for every scale a real tensor has.  The half2 are multiplied by f16(2^r) with v_pk_mul_f16: both factors are exact, so
//                                the product is f16(y) correctly rounded — into the subnormals by the hardware's own round-to-nearest-even (f16 denormals are on).
//                                Where r is clamped, y itself is beyond the range: below, k * 2^-38 rounds to 0 as y does; above, k * 2^27 is inf as y is, and code 0
//                                stays 0 (the scale is finite: no NaN from 0 * inf).  So w16 is ggml's value for all 256 x 16 (e, code) pairs, inf included.
// Hardware route (mx4_hw4): v_cvt_scalef32_pk_f16_fp4 converts the two e2m1 codes of one byte under an f32 scale.  The block's nibbles are regrouped so that a byte
//   holds two NEIGHBOURING weights (q | q >> 4 on the masked nibbles), scale = 2^(e - 127) (true e2m1 values are half the table's).
//   Measured (profiles/mxfp4_probe.txt): equal to f16(y) for every code at e <= 254, NaN for all 16 codes at e = 255, where codes 0 and 8 are zero weights.  The
//   kernels use the integer route alone; this function is kept for the probe.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mi355x {

typedef _Float16 mx4_half2_t __attribute__((ext_vector_type(2)));

struct MX4Scale {
    uint32_t t0, t1;  // magnitude bytes of codes 0 .. 3 / 4 .. 7 at this block's a
    mx4_half2_t s;    // f16(2^r), twice
};
__device__ __forceinline__ MX4Scale mx4_prep(uint32_t e) {
    const int n = (int)e - 128;
    const int a = min(max(n, -14), 12);
    const int r = min(max(n - a, -24), 15);
    const uint32_t u  = (uint32_t)(a + 14) * 4u;
    const uint32_t sb = r >= -14 ? (uint32_t)(r + 15) << 10 : 1u << (r + 24);  // f16 bits of 2^r (subnormal below 2^-14)
    MX4Scale m;
    m.t0 = 0x0A080400u + u * 0x01010100u;
    m.t1 = 0x12100E0Cu + u * 0x01010101u;
    m.s  = __builtin_bit_cast(mx4_half2_t, sb * 0x00010001u);
    return m;
}
// four codes (one per byte of q, 0 .. 15) -> weights in the order of the bytes: h01 = (w0, w1), h23 = (w2, w3).  v_perm_b32 takes selector values 0 .. 3 from its
// second operand, 4 .. 7 from its first, 0x0C gives a zero byte
__device__ __forceinline__ void mx4_w4(uint32_t q, const MX4Scale& m, mx4_half2_t& h01, mx4_half2_t& h23) {
    const uint32_t v = __builtin_amdgcn_perm(m.t1, m.t0, q & 0x07070707u) | ((q & 0x08080808u) << 4);
    h01 = __builtin_bit_cast(mx4_half2_t, __builtin_amdgcn_perm(v, v, 0x050C040Cu)) * m.s;
    h23 = __builtin_bit_cast(mx4_half2_t, __builtin_amdgcn_perm(v, v, 0x070C060Cu)) * m.s;
}
// the same through the conversion instruction; scale = the f32 2^(e - 127), see mx4_hw_scale
__device__ __forceinline__ float mx4_hw_scale(uint32_t e) { return __builtin_bit_cast(float, e ? e << 23 : 0x00400000u); }
__device__ __forceinline__ void mx4_hw4(uint32_t q, float scale, mx4_half2_t& h01, mx4_half2_t& h23) {
    const uint32_t x = q | (q >> 4);  // byte 0 = codes 0, 1; byte 2 = codes 2, 3
    h01 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(x, scale, 0);
    h23 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(x, scale, 2);
}

}  // namespace mi355x
