// kquant.hip — Linear layers whose weights are K-quant super-blocks (q2_K .. q6_K: 256 weights with packed 4- / 6-bit sub-block scales, the types the
// Q2_K / Q3_K / Q4_K_S / Q4_K_M / Q5_K_S / Q6_K GGUF files of FLUX, SD3.5 and SDXL store), kept RAW in HBM (0.33 / 0.43 / 0.5625 / 0.6875 / 0.82 B per weight).
//
// ONE weight value on every route: w16 = f16(y), y = the f32 value ggml's dequantize_row_q{2..6}_K produces with its operations in ggml's order, unfused:
//   q4_K / q5_K   d1 = d * sc;  m1 = dmin * m;  y = d1 * q - m1          q6_K   y = (d * sc) * q
//   q2_K          dl = d * (s & 15);  ml = dmin * (s >> 4);  y = dl * q - ml          q3_K   dl = d * (sc - 32);  y = dl * (q2 - (hbit ? 0 : 4))
// (kq_w8 / kq_w8s below: separately rounded operations under fp contract(off), never an FMA).  The few-row kernel and the image kernel share these decoders, so a Linear differs between its
// routes by f32 summation order only.
//
//   k_kq_gemm<KT, RB>   1 .. qgemm16_max_rows activation rows: the raw super-blocks stream from HBM once and are decoded in registers into the f16 B fragments of
//                       v_mfma_f32_32x32x16_f16; no image exists.  One super-block IS one 256-wide K segment: per segment a wave fetches the 144 / 176 / 210-byte piece
//                       of each of ITS 32 columns with coalesced 16-byte loads into a per-wave LDS strip, every lane (column n = lane % 32, k half kg = lane / 32)
//                       unpacks the 6-bit scales of its column ONCE (8 x (d1, m1) / 16 x d * sc in registers) and then walks the quant bytes in THEIR order:
//                         q4_K / q5_K  group g (64 weights), t: bytes 32 g + 8 r .. + 7 with r = 2 t + kg; their low nibbles are weights 64 g + 8 r + i (one MFMA
//                                      step), their high nibbles weights 64 g + 32 + 8 r + i (the next step); q5_K adds bit 2 g / 2 g + 1 of qh[8 r + i]
//                         q6_K         half hf (128 weights), t: ql[64 hf + 8 r ..], ql[64 hf + 32 + 8 r ..], qh[32 hf + 8 r ..] give the four steps c = 0 .. 3,
//                                      weights 128 hf + 32 c + 8 r + i
//                         q2_K / q3_K  2-bit planes in q6_K's weight order: half hf, t: the 8 bytes qs[32 hf + 8 r ..] are read ONCE and their four bit pairs
//                                      c = 0 .. 3 are the four steps, weights 128 hf + 32 c + 8 r + i; q3_K adds bit 4 hf + c of hmask[8 r + i], 8 bytes read once
//                                      per segment and run for both halves, and unpacks its six-bit scales from 12 bytes held as three dwords.  The step's
//                                      sub-block scale is 8 hf + 2 c + t: each of the 16 is needed at exactly one (hf, t, c), so it is unpacked where it is used
//                                      (4 x (dl, ml) live, not 16) at no extra work.
//                       and the A fragment of each step is read from LDS at the same permuted k offset: no lane shuffles.
//                       q6_K rows are only 2-byte aligned (210 K / 256 bytes): the fetch takes the 14 ALIGNED 16-byte granules that cover the piece (they share
//                       their first and last valid byte's granule with it, so they never touch a page the tensor does not) and the LDS reads re-align with v_alignbit.
//                       q2_K rows are 4-byte aligned (84 K / 256 bytes), q3_K rows 2-byte aligned (110 K / 256): the same rule, only granules that hold a valid
//                       byte: always 6 for q2_K (phase + 84 > 80), 7 for q3_K at phase 0 / 2 and 8 from phase 4 on.  q2_K fields are read as dwords, q3_K's
//                       through v_alignbit.  Strip stride per column: not the natural 96 / 128 bytes (24 / 32 dwords: the 32 columns of a wave would start on 8 / 2
//                       of the 64 banks) but 104 / 136 bytes = 13 / 17 x 8: 26 / 34 dwords, 2 x odd, so the 32 columns start on 32 different even banks (the
//                       stash is two 8-byte LDS stores per granule).  LDS: strips 4 x (32 x 104 + 16) = 13376 B / 4 x (32 x 136 + 16) = 17472 B, plus the A
//                       tile of 16.5 KiB per 32 rows: 47168 / 51264 B at 64-row tiles.
//                       Tile: 32 RB rows x 128 columns (4 waves x 32), next segment's global loads in flight during the MFMAs; split-K over gridDim.z into f32 slabs.
//                       A = the f16 operand image, or for 1 .. 4 rows the f32 rows themselves (SiLU and pre_scale applied while they are staged).
//   k_kq_gemv<KT, R>    1 .. 4 activation rows of the HOISTED groups (modulation / embedding Linears that share one input: one launch for all of them): a weight
//                       stream on the VALUs, lanes own 8-weight runs of the same walk, no matrix instruction (its own header below)
//   k_kq_image<KT>      raw super-blocks -> the f16 fragment-order image [col/32][K/16][64 lanes][8 halfs] of k_gemm16 (plain row order and both GEGLU orders of
//                       k_wswz_linear): a workgroup owns 32 image rows x 256 k, loads the 32 super-blocks coalesced into LDS, wave w decodes ITS group g = w
//                       (q4_K / q5_K: two sub-block scales per lane) / (half, t) = (w / 2, w % 2) (q6_K, q2_K, q3_K: four scales) and writes four whole 1 KiB fragments.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include "device_utils.h"
#include "kernels.h"
#include "ktime.h"

namespace mi355x {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

template <int KT>
struct KQ;
// BS: bytes per super-block; NGC: aligned 16-byte granules that cover one at its worst phase; CP: bytes between the columns of an LDS strip; PH: the rows
// are not 16-byte aligned (the fetch starts at the granule that holds the super-block's first byte, the LDS reads add its phase)
template <>
struct KQ<2> {
    static constexpr int BS = 84, NGC = 6, CP = 104, QS = 16, QH = 0;  // 4-byte phases: 12 + 84 = 96; 13 x 8 bytes (see the header)
    static constexpr bool PH = true;
};
template <>
struct KQ<3> {
    static constexpr int BS = 110, NGC = 8, CP = 136, QS = 32, QH = 0;  // 2-byte phases: 7 granules at phase 0 / 2, else 8 (14 + 110 = 124); 17 x 8 bytes
    static constexpr bool PH = true;
};
template <>
struct KQ<4> {
    static constexpr int BS = 144, NGC = 9, CP = 144, QS = 16, QH = 0;
    static constexpr bool PH = false;
};
template <>
struct KQ<5> {
    static constexpr int BS = 176, NGC = 11, CP = 176, QS = 48, QH = 16;
    static constexpr bool PH = false;
};
template <>
struct KQ<6> {
    static constexpr int BS = 210, NGC = 14, CP = 224, QS = 0, QH = 128;  // NGC: aligned granules covering 210 bytes at any even phase (14 + 210 = 224)
    static constexpr bool PH = true;
};
// the granule gr of a super-block at phase ph holds one of its bytes (q3_K alone has a granule that some phases do not need)
template <int KT>
__device__ __forceinline__ bool kq_granule_valid(int gr, uint32_t ph) {
    return KT != 3 || gr * 16 < (int)ph + KQ<KT>::BS;
}
// a fetched granule into its place in a strip: CP is a multiple of 16 for q4_K .. q6_K, of 8 only for q2_K / q3_K (two 8-byte stores)
template <int KT>
__device__ __forceinline__ void kq_stash(char* strip, int idx, const u32x4_t& v) {
    if constexpr (KQ<KT>::CP == KQ<KT>::NGC * 16) {
        *(u32x4_t*)(strip + idx * 16) = v;
    } else {
        const int col = idx / KQ<KT>::NGC, gr = idx - col * KQ<KT>::NGC;
        uint2* q = (uint2*)(strip + col * KQ<KT>::CP + gr * 16);
        q[0]     = make_uint2(v[0], v[1]);
        q[1]     = make_uint2(v[2], v[3]);
    }
}

// 8 bytes at byte offset off of an LDS strip: 8-byte aligned (q4_K / q5_K fields), or 2-byte aligned (q6_K) through three dwords and v_alignbit
template <bool ALIGNED>
__device__ __forceinline__ void kq_ld8(const char* strip, uint32_t off, uint32_t& a, uint32_t& b) {
    if (ALIGNED) {
        const uint2 v = *(const uint2*)(strip + off);
        a = v.x;
        b = v.y;
    } else {
        const char* p     = strip + (off & ~3u);
        const uint32_t sh = (off & 2u) * 8u;
        const uint32_t r0 = *(const uint32_t*)p, r1 = *(const uint32_t*)(p + 4), r2 = *(const uint32_t*)(p + 8);
        a = __builtin_amdgcn_alignbit(r1, r0, sh);
        b = __builtin_amdgcn_alignbit(r2, r1, sh);
    }
}

// eight quants (one per byte of a, b) -> f16(d1 * q - m1), each operation rounded on its own
__device__ __forceinline__ half8_t kq_w8(uint32_t a, uint32_t b, float d1, float m1) {
#pragma clang fp contract(off)  // plain operators under this pragma (the rounding intrinsics of the HIP headers are inlined WITH their contract flag: v_fma_mix)
    half8_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float pa = d1 * (float)((a >> (8 * j)) & 0xFFu), pb = d1 * (float)((b >> (8 * j)) & 0xFFu);
        o[j]     = (_Float16)(pa - m1);
        o[4 + j] = (_Float16)(pb - m1);
    }
    return o;
}
// q6_K: eight 6-bit values -> f16(ds * (v - 32)), ds = d * sc already rounded; q3_K: eight 3-bit values, BIAS 4
template <int BIAS = 32>
__device__ __forceinline__ half8_t kq_w8s(uint32_t a, uint32_t b, float ds) {
#pragma clang fp contract(off)  // plain operators under this pragma (the rounding intrinsics of the HIP headers are inlined WITH their contract flag: v_fma_mix)
    half8_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float qa = (float)((a >> (8 * j)) & 0xFFu) - (float)BIAS, qb = (float)((b >> (8 * j)) & 0xFFu) - (float)BIAS;
        o[j]     = (_Float16)(ds * qa);
        o[4 + j] = (_Float16)(ds * qb);
    }
    return o;
}

// q4_K / q5_K header of the super-block at blk (16-byte aligned): d, dmin and the 12 scale bytes as three dwords
struct KQHead {
    float d, dmin;
    uint32_t s0, s1, s2;
};
__device__ __forceinline__ KQHead kq_head45(const char* blk) {
    const u32x4_t h = *(const u32x4_t*)blk;
    KQHead r;
    r.d    = (float)__builtin_bit_cast(_Float16, (uint16_t)(h[0] & 0xFFFFu));
    r.dmin = (float)__builtin_bit_cast(_Float16, (uint16_t)(h[0] >> 16));
    r.s0 = h[1];
    r.s1 = h[2];
    r.s2 = h[3];
    return r;
}
// get_scale_min_k4 of sub-block j on the three dwords: bytes 0..3 hold sc 0..3 (6 bits) + the top 2 bits of sc 4..7, bytes 4..7 the same for m, bytes 8..11 the
// low 4 bits of sc 4..7 (low nibble) and m 4..7 (high nibble)
__device__ __forceinline__ void kq_scale45(const KQHead& h, int j, float& d1, float& m1) {
    const int i = (j & 3) * 8;
    uint32_t sc, mn;
    if (j < 4) {
        sc = (h.s0 >> i) & 63u;
        mn = (h.s1 >> i) & 63u;
    } else {
        sc = ((h.s2 >> i) & 0xFu) | (((h.s0 >> (i + 6)) & 3u) << 4);
        mn = ((h.s2 >> (i + 4)) & 0xFu) | (((h.s1 >> (i + 6)) & 3u) << 4);
    }
    d1 = __fmul_rn(h.d, (float)sc);
    m1 = __fmul_rn(h.dmin, (float)mn);
}
// group g (weights 64 g .. 64 g + 63), run r (0..3) of a q4_K / q5_K super-block at strip + off: lo = weights 64 g + 8 r + i, hi = weights 64 g + 32 + 8 r + i
template <int KT>
__device__ __forceinline__ void kq_dec45(const char* strip, uint32_t off, int g, int r, uint32_t ha, uint32_t hb, float d1lo, float m1lo, float d1hi, float m1hi, half8_t& lo,
                                         half8_t& hi) {
    uint32_t qa, qb;
    kq_ld8<true>(strip, off + KQ<KT>::QS + 32 * g + 8 * r, qa, qb);
    uint32_t la = qa & 0x0F0F0F0Fu, lb = qb & 0x0F0F0F0Fu, ua = (qa >> 4) & 0x0F0F0F0Fu, ub = (qb >> 4) & 0x0F0F0F0Fu;
    if (KT == 5) {  // ha, hb: qh[8 r .. 8 r + 7]; bit 2 g is the fifth bit of the low-nibble weight, bit 2 g + 1 of the high-nibble weight
        la |= ((ha >> (2 * g)) & 0x01010101u) << 4;
        lb |= ((hb >> (2 * g)) & 0x01010101u) << 4;
        ua |= ((ha >> (2 * g + 1)) & 0x01010101u) << 4;
        ub |= ((hb >> (2 * g + 1)) & 0x01010101u) << 4;
    }
    lo = kq_w8(la, lb, d1lo, m1lo);
    hi = kq_w8(ua, ub, d1hi, m1hi);
}
// half hf, run r of a q6_K super-block at strip + off (any even off): o[c] = weights 128 hf + 32 c + 8 r + i; ds[c] = d * scales[8 hf + 2 c + r / 2]
__device__ __forceinline__ void kq_dec6(const char* strip, uint32_t off, int hf, int r, const float (&ds)[4], half8_t (&o)[4]) {
    uint32_t a0, b0, a1, b1, ha, hb;
    kq_ld8<false>(strip, off + 64 * hf + 8 * r, a0, b0);
    kq_ld8<false>(strip, off + 64 * hf + 32 + 8 * r, a1, b1);
    kq_ld8<false>(strip, off + 128 + 32 * hf + 8 * r, ha, hb);
    const uint32_t m4 = 0x0F0F0F0Fu, m2 = 0x03030303u;
    o[0] = kq_w8s((a0 & m4) | ((ha & m2) << 4), (b0 & m4) | ((hb & m2) << 4), ds[0]);
    o[1] = kq_w8s((a1 & m4) | (((ha >> 2) & m2) << 4), (b1 & m4) | (((hb >> 2) & m2) << 4), ds[1]);
    o[2] = kq_w8s(((a0 >> 4) & m4) | (((ha >> 4) & m2) << 4), ((b0 >> 4) & m4) | (((hb >> 4) & m2) << 4), ds[2]);
    o[3] = kq_w8s(((a1 >> 4) & m4) | (((ha >> 6) & m2) << 4), ((b1 >> 4) & m4) | (((hb >> 6) & m2) << 4), ds[3]);
}
__device__ __forceinline__ float kq_ds6(const char* strip, uint32_t off, int idx) {
    const float d = (float)*(const _Float16*)(strip + off + 208);
    return __fmul_rn(d, (float)(int)*(const int8_t*)(strip + off + 192 + idx));
}

// ---- q2_K {u8 scales[16]; u8 qs[64]; f16 d; f16 dmin} at any 4-byte phase, q3_K {u8 hmask[32]; u8 qs[64]; u8 scales[12]; f16 d} at any 2-byte phase
// the packed sub-block scales of the super-block at strip + off as aligned dwords (q2_K: 16 bytes, q3_K: 12), d and dmin
struct KQHead23 {
    float d, dmin;
    uint32_t s[4];
};
template <int KT>
__device__ __forceinline__ KQHead23 kq_head23(const char* strip, uint32_t off) {
    KQHead23 h;
    if (KT == 2) {
        const uint32_t* b = (const uint32_t*)(strip + off);
#pragma unroll
        for (int i = 0; i < 4; ++i) h.s[i] = b[i];
        const uint32_t dd = b[20];
        h.d    = (float)__builtin_bit_cast(_Float16, (uint16_t)(dd & 0xFFFFu));
        h.dmin = (float)__builtin_bit_cast(_Float16, (uint16_t)(dd >> 16));
    } else {
        const uint32_t* b = (const uint32_t*)(strip + ((off + 96) & ~3u));
        const uint32_t sh = (off & 2u) * 8u, r0 = b[0], r1 = b[1], r2 = b[2], r3 = b[3];
        h.s[0] = __builtin_amdgcn_alignbit(r1, r0, sh);
        h.s[1] = __builtin_amdgcn_alignbit(r2, r1, sh);
        h.s[2] = __builtin_amdgcn_alignbit(r3, r2, sh);
        h.s[3] = 0;
        h.d    = (float)*(const _Float16*)(strip + off + 108);
        h.dmin = 0.f;
    }
    return h;
}
// sub-block j (16 weights): q2_K dl = d * (scales[j] & 0xF), ml = dmin * (scales[j] >> 4); q3_K dl = d * (six-bit scale j - 32), its low four bits the low
// (j < 8) or high nibble of byte j & 7, its high two bits at bit 2 (j >> 2) of byte 8 + (j & 3)
template <int KT>
__device__ __forceinline__ void kq_scale23(const KQHead23& h, int j, float& dl, float& ml) {
    if (KT == 2) {
        // (selects, not h.s[j >> 2]: in the image kernel j depends on the wave, and an indexed private array is moved to LDS)
        const uint32_t sw = (j & 8) ? ((j & 4) ? h.s[3] : h.s[2]) : ((j & 4) ? h.s[1] : h.s[0]);
        const uint32_t sb = (sw >> (8 * (j & 3))) & 0xFFu;
        dl = __fmul_rn(h.d, (float)(sb & 0xFu));
        ml = __fmul_rn(h.dmin, (float)(sb >> 4));
    } else {
        const uint32_t lo = (((j & 4) ? h.s[1] : h.s[0]) >> (8 * (j & 3) + (j < 8 ? 0 : 4))) & 0xFu, hi = (h.s[2] >> (8 * (j & 3) + 2 * (j >> 2))) & 3u;
        dl = __fmul_rn(h.d, (float)((int)(lo | (hi << 4)) - 32));
        ml = 0.f;
    }
}
// half hf, run r = 2 t + kg of the super-block at strip + off: the 8 bytes qs[32 hf + 8 r ..] hold four MFMA steps as their four bit pairs, o[c] = weights
// 128 hf + 32 c + 8 r + i with sub-block scale 8 hf + 2 c + t.  q3_K: ha, hb = hmask[8 r .. 8 r + 7] (the same bytes for both halves), third bit = bit 4 hf + c
template <int KT>
__device__ __forceinline__ void kq_dec23(const char* strip, uint32_t off, const KQHead23& h, int hf, int t, int r, uint32_t ha, uint32_t hb, half8_t (&o)[4]) {
    const uint32_t m2 = 0x03030303u, m1 = 0x01010101u;
    uint32_t qa, qb;
    if (KT == 2) {  // 4-byte aligned: two dwords
        const uint32_t* q = (const uint32_t*)(strip + off + KQ<2>::QS + 32 * hf + 8 * r);
        qa = q[0];
        qb = q[1];
    } else {
        kq_ld8<false>(strip, off + KQ<3>::QS + 32 * hf + 8 * r, qa, qb);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float dl, ml;
        kq_scale23<KT>(h, 8 * hf + 2 * c + t, dl, ml);
        const uint32_t va = (qa >> (2 * c)) & m2, vb = (qb >> (2 * c)) & m2;
        if (KT == 2) o[c] = kq_w8(va, vb, dl, ml);
        else o[c] = kq_w8s<4>(va | (((ha >> (4 * hf + c)) & m1) << 2), vb | (((hb >> (4 * hf + c)) & m1) << 2), dl);
    }
}

// =====================================================================================================
// k_kq_gemm
// =====================================================================================================
struct KQArgs {
    const char* W;
    int64_t row_bytes;
    const _Float16* A;  // f16 operand image [rows][lda], or nullptr:
    int64_t lda;
    const float* x32;   // ... the f32 activation rows (row stride xs floats), staged as f16(silu?(x) * pre_scale)
    int64_t xs;
    float pre_scale;
    int pre_silu;
    float* dst;
    int64_t ldd;
    _Float16* dst16;
    int64_t ldd16;
    const float* bias;
    const float* residual;
    const float* gate;
    int gate_L, gelu;
    float scale;
    int R, M;
    int nseg, nseg_slice;
    int64_t slab;
    int a_runL, a_runS;
};

template <int KT, int RB>
__global__ __launch_bounds__(256) void k_kq_gemm(KQArgs g) {
    constexpr int BS  = KQ<KT>::BS;
    constexpr int NGC = KQ<KT>::NGC;
    constexpr int CP  = KQ<KT>::CP;        // bytes between the columns of a strip
    constexpr int NGW = 32 * NGC;          // granules of a wave's strip
    constexpr int NLW = (NGW + 63) / 64;   // loads per lane: 3 / 4 (q2_K / q3_K), 5 / 6 / 7
    constexpr int RT  = RB * 32;
    constexpr int AS  = 256 * 2 + 16;      // bytes between A rows in LDS
    constexpr int NLA = RT * 32 / 256;     // A granules per thread
    __shared__ __attribute__((aligned(16))) char As[RT * AS];
    __shared__ __attribute__((aligned(16))) char Wsm[4][32 * CP + 16];  // (+ 16: the third dword of an unaligned 8-byte read at a strip's end)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 31, kg = lane >> 5;
    char* Ws           = Wsm[wave];
    const int64_t row0 = (int64_t)blockIdx.x * RT;
    const int colw     = (int)blockIdx.y * 128 + wave * 32;
    const int seg0     = (int)blockIdx.z * g.nseg_slice;
    const int seg1     = min(g.nseg, seg0 + g.nseg_slice);
    const char* mycol  = g.W + (int64_t)min(colw + n, g.M - 1) * g.row_bytes;  // this lane's column (q6_K: its phase inside the strip)

    float16_t acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[rb][i] = 0.f;

    u32x4_t wreg[NLW], areg[NLA];
    auto a_phys = [&](int64_t r) -> int64_t {
        return g.a_runL > 0 ? (int64_t)((uint32_t)r / (uint32_t)g.a_runL) * g.a_runS + (uint32_t)r % (uint32_t)g.a_runL : r;
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < NLW; ++i) {
            const int idx = i * 64 + lane;
            if (idx < NGW) kq_stash<KT>(Ws, idx, wreg[i]);
        }
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int idx = i * 256 + (int)threadIdx.x;
            *(u32x4_t*)(As + (idx >> 5) * AS + (idx & 31) * 16) = areg[i];
        }
    };
    auto fetch = [&](int seg) {
#pragma unroll
        for (int i = 0; i < NLW; ++i) {
            const int idx = i * 64 + lane;
            const int col = idx / NGC, gr = idx - col * NGC;
            const int cc  = min(colw + col, g.M - 1);
            wreg[i]       = (u32x4_t){0, 0, 0, 0};
            if (idx < NGW) {
                const char* p     = g.W + (int64_t)cc * g.row_bytes + (int64_t)seg * BS;
                const uint32_t ph = KQ<KT>::PH ? (uint32_t)((uintptr_t)p & 15) : 0;
                if (kq_granule_valid<KT>(gr, ph)) wreg[i] = *(const u32x4_t*)(p - ph + gr * 16);
            }
        }
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int idx     = i * 256 + (int)threadIdx.x;
            const int row     = idx >> 5, gr = idx & 31;
            const int64_t grw = row0 + row;
            areg[i]           = (u32x4_t){0, 0, 0, 0};
            if (grw < g.R) {
                if (g.A) {
                    areg[i] = *(const u32x4_t*)(g.A + a_phys(grw) * g.lda + (int64_t)seg * 256 + gr * 8);
                } else {
                    const float* xr = g.x32 + grw * g.xs + (int64_t)seg * 256 + gr * 8;
                    const float4 a = *(const float4*)xr, b = *(const float4*)(xr + 4);
                    float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                    half8_t h;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float u = g.pre_silu ? act_apply<UN_SILU>(v[j]) : v[j];
                        h[j]          = (_Float16)(u * g.pre_scale);
                    }
                    areg[i] = __builtin_bit_cast(u32x4_t, h);
                }
            }
        }
    };
    auto step = [&](const half8_t& bf, int k0) {
        half8_t af[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) af[rb] = *(const half8_t*)(As + (rb * 32 + n) * AS + k0 * 2);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[rb], bf, acc[rb], 0, 0, 0);
    };
    auto compute_seg = [&](int seg) {
        if constexpr (KT == 6) {
            const uint32_t off = (uint32_t)n * CP + (uint32_t)((uintptr_t)(mycol + (int64_t)seg * BS) & 15);
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int r = 2 * t + kg;
                    float ds[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) ds[c] = kq_ds6(Ws, off, 8 * hf + 2 * c + t);
                    half8_t o[4];
                    kq_dec6(Ws, off, hf, r, ds, o);
#pragma unroll
                    for (int c = 0; c < 4; ++c) step(o[c], 128 * hf + 32 * c + 8 * r);
                }
        } else if constexpr (KT == 2 || KT == 3) {
            const uint32_t off = (uint32_t)n * CP + (uint32_t)((uintptr_t)(mycol + (int64_t)seg * BS) & 15);
            const KQHead23 h   = kq_head23<KT>(Ws, off);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int r = 2 * t + kg;
                uint32_t ha = 0, hb = 0;
                if (KT == 3) kq_ld8<false>(Ws, off + 8 * r, ha, hb);  // once per segment and run: both halves
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    half8_t o[4];
                    kq_dec23<KT>(Ws, off, h, hf, t, r, ha, hb, o);
#pragma unroll
                    for (int c = 0; c < 4; ++c) step(o[c], 128 * hf + 32 * c + 8 * r);
                }
            }
        } else {
            const uint32_t off = (uint32_t)n * CP;
            const KQHead h     = kq_head45(Ws + off);
            float d1[8], m1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) kq_scale45(h, j, d1[j], m1[j]);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int r = 2 * t + kg;
                uint32_t ha = 0, hb = 0;
                if (KT == 5) kq_ld8<true>(Ws, off + KQ<KT>::QH + 8 * r, ha, hb);
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    half8_t lo, hi;
                    kq_dec45<KT>(Ws, off, gq, r, ha, hb, d1[2 * gq], m1[2 * gq], d1[2 * gq + 1], m1[2 * gq + 1], lo, hi);
                    step(lo, 64 * gq + 8 * r);
                    step(hi, 64 * gq + 32 + 8 * r);
                }
            }
        }
    };
    if (seg0 < seg1) fetch(seg0);
    for (int seg = seg0; seg < seg1; ++seg) {
        __syncthreads();  // every wave is done reading the previous segment
        stash();
        __syncthreads();
        if (seg + 1 < seg1) fetch(seg + 1);  // in flight during the MFMAs below
        compute_seg(seg);
    }
    // ---- store: register r of a 32x32 block holds row (r & 3) + 8 (r >> 2) + 4 kg, lanes run along columns
    const int col = colw + n;
    if (col >= g.M) return;
    const float bias = (g.bias && g.slab == 0) ? g.bias[col] : 0.f;
    float* dst       = g.dst + (g.slab > 0 ? (int64_t)blockIdx.z * g.slab : 0);
    const int mode   = g.slab > 0 ? 0 : g.gelu ? 1 : g.gate ? 2 : g.residual ? 3 : 0;  // workgroup-uniform
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int rbase = (int)row0 + rb * 32 + 4 * kg;
        if ((int)row0 + rb * 32 >= g.R) break;
        if (mode == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rbase + (r & 3) + 8 * (r >> 2);
                if (row < g.R) dst[(int64_t)row * g.ldd + col] = acc[rb][r] * g.scale + bias;
            }
        } else if (mode == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rbase + (r & 3) + 8 * (r >> 2);
                if (row < g.R) g.dst16[(int64_t)row * g.ldd16 + col] = (_Float16)act_apply<UN_GELU>(acc[rb][r] * g.scale + bias);
            }
        } else {
            float rv[16], gv[16];  // fetched together from clamped rows (cf. k_qgemm16)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = min(rbase + (r & 3) + 8 * (r >> 2), g.R - 1);
                rv[r]         = g.residual[(int64_t)row * g.ldd + col];
                gv[r]         = mode == 2 ? g.gate[(int64_t)((uint32_t)row / (uint32_t)g.gate_L) * g.M + col] : 1.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rbase + (r & 3) + 8 * (r >> 2);
                if (row < g.R) dst[(int64_t)row * g.ldd + col] = (acc[rb][r] * g.scale + bias) * gv[r] + rv[r];
            }
        }
    }
}

// =====================================================================================================
// k_kq_gemv
// =====================================================================================================
// 1 .. 4 activation rows against raw K-quant rows as a pure weight stream: no matrix instruction, no workgroup barrier inside the K loop.
//   lanes     a super-block is cut into lane TASKS along its quant bytes, so that a lane reads its bytes once and one decode serves all R activation rows:
//               q4_K / q5_K  16 tasks (g, r): bytes qs[32 g + 8 r ..] -> weights 64 g + 8 r + i (low nibbles) and 64 g + 32 + 8 r + i (high): 16 weights
//               q6_K          8 tasks (hf, r): ql[64 hf + 8 r ..], ql[64 hf + 32 + 8 r ..], qh[32 hf + 8 r ..] -> weights 128 hf + 32 c + 8 r + i, c = 0 .. 3
//               q2_K / q3_K   8 tasks (hf, r): qs[32 hf + 8 r ..] -> the same 32 weights from its four bit pairs (q3_K: + hmask[8 r ..])
//             (the walk of k_kq_gemm above with (t, kg) = (r / 2, r % 2); each sub-block scale is unpacked by the task that uses it).  Lane l of a wave takes
//             task l % TPS of super-block l / TPS of the step: a wave step covers SPS = 4 (q4_K / q5_K) or 8 super-blocks of ONE weight row.
//   waves     a wave owns 4 consecutive weight rows (= output columns; members of a grouped launch are multiples of 4 rows, so the four belong to one member) and
//             walks K in steps; a workgroup's four waves take 1 .. 4 such groups each (gpw: 64 columns per workgroup once that still gives 1024 workgroups), so
//             the staged activation rows are amortised over 16 .. 64 columns.
//   weights   the SPS super-blocks of a row step are contiguous in HBM: the wave copies the ALIGNED 16-byte granules that hold one of their bytes (phase = address
//             & 15 for the 2- / 4-byte aligned rows of q2_K / q3_K / q6_K: the first and last granule share a valid byte with the row, so no granule lies outside
//             the tensor) linearly into its private strip, one granule per lane and load: 36 / 44 granules (q4_K / q5_K), <= 43 / 56 (q2_K / q3_K), <= 106 (q6_K, two
//             loads).  The loads of all four rows are issued before the first is consumed, and a row's registers are refilled with the NEXT step's granules as soon
//             as they are stashed: four row steps are in flight per wave at any time.  The strip is private to the wave: wavefront-scope fences only.
//             Strip stride between super-blocks = their stride in memory (a linear copy cannot pad it): 36 / 44 dwords (q4_K / q5_K: a task's 8 bytes are dwords
//             4 + 2 u of its super-block, the 16 tasks 32 consecutive dwords; the two super-blocks of a 32-lane half start 36 / 44 dwords apart, so 28 / 20 of
//             their 32 banks are distinct); 21 / 27.5 / 52.5 dwords (q2_K / q3_K / q6_K: a super-block's 8 tasks read two runs of 8 consecutive dwords 8 apart,
//             the 8 super-blocks start on banks 21 j / 27.5 j / 52.5 j mod 64: odd or half-odd strides, no two on the same bank).
//   x         staged once per workgroup into LDS as f16(silu?(x) * pre_scale) (k_qgemv's rounding point).  A task reads 16-byte chunks (8 k) 8 g + r and + 4
//             (q4_K / q5_K) or 16 hf + 4 c + r: chunk ci of a row sits at slot ci ^ (bit 4 of ci << 2) ^ (bit 5 of ci << 3), so the 16 lanes of a quarter wave (one
//             super-block of 16 tasks, or two of 8) read 16 different 16-byte slots modulo 256 bytes: all 64 banks once.  Read once per step, used by all four rows.
//   sums      w16 from the shared decoders, (float)w16 * (float)x16 accumulated with f32 FMAs (v_fma_mix_f32: the conversions ride in the FMA) in two chains per
//             (row, activation row); v_dot2_f32_f16 would halve these R operations per weight, but how it treats subnormal f16 operands was not verified
//             against the MFMA's, and the decode (about 4 operations per weight), not the FMAs, is the larger share.  wave_sum_transpose over the 4 R sums.
template <int KT>
struct KQV {
    static constexpr int TPS  = (KT == 4 || KT == 5) ? 16 : 8;  // lane tasks per super-block
    static constexpr int SPS  = 64 / TPS;                       // super-blocks of a row per wave step
    static constexpr int NCH  = 32 / TPS;                       // 8-weight runs per task
    static constexpr int SEGB = SPS * KQ<KT>::BS;               // bytes of a full row step
    static constexpr int NG   = (SEGB + (KQ<KT>::PH ? 15 : 0) + 15) / 16;
    static constexpr int NLD  = (NG + 63) / 64;                 // loads per lane and row step
};
constexpr int KQV_CPW = 4;
__device__ __forceinline__ int kqv_xslot(int ci) { return ci ^ (((ci >> 4) & 1) << 2) ^ (((ci >> 5) & 1) << 3); }

struct KQVArgs {
    QGArgs q;
    int gpw;  // column groups of 4 per wave
};

template <int KT, int R>
__global__ __launch_bounds__(256) void k_kq_gemv(KQVArgs a) {
    using V = KQV<KT>;
    const QGArgs& g = a.q;
    constexpr int BS = KQ<KT>::BS, CPW = KQV_CPW, NLD = V::NLD, TPS = V::TPS, SPS = V::SPS, NCH = V::NCH;
    __shared__ __attribute__((aligned(16))) char strip[4][NLD * 64 * 16 + 16];  // (+ 16: the third dword of an unaligned 8-byte read at the strip's end)
    extern __shared__ __attribute__((aligned(16))) char xlds[];                 // [R][K] halfs, chunk ci at slot kqv_xslot(ci)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char* my       = strip[wave];
    const int nsb  = g.K / 256;
    const int nseg = (nsb + SPS - 1) / SPS;
    for (int c8 = threadIdx.x; c8 < g.K / 8; c8 += 256) {  // all R rows of a chunk column in flight together
        float4 xa[R], xb[R];
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const float* xr = g.x + (int64_t)(t < g.rows ? t : 0) * g.xs + c8 * 8;
            xa[t]           = *(const float4*)xr;
            xb[t]           = *(const float4*)(xr + 4);
        }
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const float v[8] = {xa[t].x, xa[t].y, xa[t].z, xa[t].w, xb[t].x, xb[t].y, xb[t].z, xb[t].w};
            half8_t h;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float u = g.pre_silu ? act_apply<UN_SILU>(v[i]) : v[i];
                h[i]          = (_Float16)(u * g.pre_scale);
            }
            *(half8_t*)(xlds + ((size_t)t * g.K + (size_t)kqv_xslot(c8) * 8) * 2) = h;
        }
    }
    __syncthreads();
    const int j = lane / TPS, u = lane % TPS;  // this lane's super-block of the step and its task
    const int hi2 = u >> 2, r = u & 3;         // (g, r) / (hf, r)
    for (int it = 0; it < a.gpw; ++it) {
        const int col0 = ((int)blockIdx.x * a.gpw * 4 + it * 4 + wave) * CPW;
        if (col0 >= g.M) break;
        // this wave's weight rows: of the single weight, or of the member of a grouped launch that owns output column col0; Wb / bb are biased so that they
        // are indexed by the GLOBAL column (k_qgemv)
        const char* Wb  = g.W;
        const float* bb = g.bias;
        if (g.members) {
            int m = 0;  // (a linear scan of the table, once per column group: the planner's groups have 3 .. a few dozen members; a binary search if they ever grow)
            while (m + 1 < g.n_members && g.members[m + 1].start <= col0) ++m;
            const QGMember mem = g.members[m];
            Wb = mem.W - (int64_t)mem.start * g.row_bytes;
            bb = mem.bias ? mem.bias - mem.start : nullptr;
        }
        float acc[CPW][R];
#pragma unroll
        for (int c = 0; c < CPW; ++c)
#pragma unroll
            for (int t = 0; t < R; ++t) acc[c][t] = 0.f;
        u32x4_t gl[CPW][NLD];
        auto rowp = [&](int c, int seg) { return Wb + (int64_t)min(col0 + c, g.M - 1) * g.row_bytes + (int64_t)seg * V::SEGB; };  // (the clamp only bites in a single weight's last group)
        auto fetch = [&](int c, int seg) {
            const char* p     = rowp(c, seg);
            const uint32_t ph = KQ<KT>::PH ? (uint32_t)((uintptr_t)p & 15) : 0;
            const int ng      = (int)(ph + (uint32_t)min(SPS, nsb - seg * SPS) * BS + 15) / 16;  // granules that hold a byte of this row step
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int gidx = i * 64 + lane;
                gl[c][i]       = gidx < ng ? *(const u32x4_t*)(p - ph + (int64_t)gidx * 16) : (u32x4_t){0, 0, 0, 0};
            }
        };
#pragma unroll
        for (int c = 0; c < CPW; ++c) fetch(c, 0);
        for (int seg = 0; seg < nseg; ++seg) {
            const int sb    = seg * SPS + j;
            const bool have = sb < nsb;
            // the activation values of this lane's task: registers, shared by the four weight rows
            half8_t xh[R][NCH];
#pragma unroll
            for (int t = 0; t < R; ++t)
#pragma unroll
                for (int cc = 0; cc < NCH; ++cc) {
                    const int ci = 32 * (have ? sb : 0) + (TPS == 16 ? 8 * hi2 + 4 * cc + r : 16 * hi2 + 4 * cc + r);
                    xh[t][cc]    = *(const half8_t*)(xlds + ((size_t)t * g.K + (size_t)kqv_xslot(ci) * 8) * 2);
                }
#pragma unroll
            for (int c = 0; c < CPW; ++c) {
                const uint32_t ph = KQ<KT>::PH ? (uint32_t)((uintptr_t)rowp(c, seg) & 15) : 0;
                // LDS operations of one wave execute in order: the wavefront-scope fences only stop the compiler from moving the task reads across other
                // lanes' stores (k_qgemv)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < NLD; ++i) *(u32x4_t*)(my + (i * 64 + lane) * 16) = gl[c][i];
                if (seg + 1 < nseg) fetch(c, seg + 1);  // in flight for a whole step
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (have) {  // (a lane past the row's last super-block would decode stale strip bytes)
                    const uint32_t off = ph + (uint32_t)j * BS;
                    half8_t o[NCH];
                    if constexpr (KT == 4 || KT == 5) {
                        const KQHead h = kq_head45(my + off);
                        float d1lo, m1lo, d1hi, m1hi;
                        kq_scale45(h, 2 * hi2, d1lo, m1lo);
                        kq_scale45(h, 2 * hi2 + 1, d1hi, m1hi);
                        uint32_t ha = 0, hb = 0;
                        if (KT == 5) kq_ld8<true>(my, off + KQ<KT>::QH + 8 * r, ha, hb);
                        kq_dec45<KT>(my, off, hi2, r, ha, hb, d1lo, m1lo, d1hi, m1hi, o[0], o[1]);
                    } else if constexpr (KT == 6) {
                        float ds[4];
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) ds[cc] = kq_ds6(my, off, 8 * hi2 + 2 * cc + (r >> 1));
                        kq_dec6(my, off, hi2, r, ds, o);
                    } else {
                        const KQHead23 h = kq_head23<KT>(my, off);
                        uint32_t ha = 0, hb = 0;
                        if (KT == 3) kq_ld8<false>(my, off + 8 * r, ha, hb);
                        kq_dec23<KT>(my, off, h, hi2, r >> 1, r, ha, hb, o);
                    }
#pragma unroll
                    for (int t = 0; t < R; ++t) {
                        float sa = 0.f, sb2 = 0.f;
#pragma unroll
                        for (int cc = 0; cc < NCH; ++cc)
#pragma unroll
                            for (int i = 0; i < 8; i += 2) {
                                sa  = fmaf((float)o[cc][i], (float)xh[t][cc][i], sa);
                                sb2 = fmaf((float)o[cc][i + 1], (float)xh[t][cc][i + 1], sb2);
                            }
                        acc[c][t] += sa + sb2;
                    }
                }
            }
        }
        // ---- cross-lane sums and store: value c * R + t ends up complete in the lanes of group (c * R + t)
        constexpr int NV  = CPW * R;
        constexpr int GRP = 64 / NV;
        float v[NV];
#pragma unroll
        for (int c = 0; c < CPW; ++c)
#pragma unroll
            for (int t = 0; t < R; ++t) v[c * R + t] = acc[c][t];
        const float tot = wave_sum_transpose<NV>(v, lane);
        const int idx = lane / GRP, c = idx / R, t = idx - c * R, col = col0 + c;
        if ((lane & (GRP - 1)) == 0 && t < g.rows && col < g.M) {
            float out = tot * g.scale + (bb ? bb[col] : 0.f);
            if (g.residual) out += g.residual[(int64_t)t * g.ldd + col];
            g.dst[(int64_t)t * g.ldd + col] = out;
        }
    }
}

// =====================================================================================================
// k_kq_image
// =====================================================================================================
// source row of image row (32-row block rb, n) under k_wswz_linear's three orders; >= R: a zero row
__device__ __forceinline__ int64_t kq_image_row(int64_t rb, int n, int64_t R, int64_t geglu_inner) {
    if (geglu_inner > 0) {  // 128-column value / gate pairing
        const int64_t t = rb >> 2, q = rb & 3, b = (2 * t + (q >> 1)) * 32;
        return b >= geglu_inner ? R : (q & 1) * geglu_inner + b + n;
    }
    if (geglu_inner < 0) {  // 16-column interleave
        const int64_t inner = -geglu_inner, out = rb * 16 + (n & 15);
        return out < inner ? ((n & 16) ? inner : 0) + out : R;
    }
    return rb * 32 + n;
}

template <int KT>
__global__ __launch_bounds__(256) void k_kq_image(half8_t* __restrict__ dst, const char* __restrict__ W, int64_t row_bytes, int64_t R, int64_t kfr, int64_t geglu_inner) {
    constexpr int BS  = KQ<KT>::BS;
    constexpr int NGC = KQ<KT>::NGC;
    constexpr int CP  = KQ<KT>::CP;
    constexpr int NGW = 32 * NGC;
    __shared__ __attribute__((aligned(16))) char Ws[32 * CP + 16];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 31, hi = lane >> 5;
    const int64_t rb = blockIdx.x;
    const int seg    = blockIdx.y;
    for (int idx = threadIdx.x; idx < NGW; idx += 256) {
        const int col    = idx / NGC, gr = idx - col * NGC;
        const int64_t rr = min(kq_image_row(rb, col, R, geglu_inner), R - 1);
        const char* p     = W + rr * row_bytes + (int64_t)seg * BS;
        const uint32_t ph = KQ<KT>::PH ? (uint32_t)((uintptr_t)p & 15) : 0;
        if (kq_granule_valid<KT>(gr, ph)) kq_stash<KT>(Ws, idx, *(const u32x4_t*)(p - ph + gr * 16));
    }
    __syncthreads();
    const int64_t src = kq_image_row(rb, n, R, geglu_inner);
    const bool real   = src < R;
    half8_t* out      = dst + (rb * kfr + (int64_t)seg * 16) * 64 + lane;
    const half8_t z   = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (KT == 6) {
        const uint32_t off = (uint32_t)n * CP + (uint32_t)((uintptr_t)(W + min(src, R - 1) * row_bytes + (int64_t)seg * BS) & 15);
        const int hf = wave >> 1, t = wave & 1, r = 2 * t + hi;
        float ds[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) ds[c] = kq_ds6(Ws, off, 8 * hf + 2 * c + t);
        half8_t o[4];
        kq_dec6(Ws, off, hf, r, ds, o);
#pragma unroll
        for (int c = 0; c < 4; ++c) out[(8 * hf + 2 * c + t) * 64] = real ? o[c] : z;  // weights 128 hf + 32 c + 16 t + 8 hi + i
    } else if constexpr (KT == 2 || KT == 3) {  // the same (half, t) per wave and the same four fragments
        const uint32_t off = (uint32_t)n * CP + (uint32_t)((uintptr_t)(W + min(src, R - 1) * row_bytes + (int64_t)seg * BS) & 15);
        const int hf = wave >> 1, t = wave & 1, r = 2 * t + hi;
        const KQHead23 h = kq_head23<KT>(Ws, off);
        uint32_t ha = 0, hb = 0;
        if (KT == 3) kq_ld8<false>(Ws, off + 8 * r, ha, hb);
        half8_t o[4];
        kq_dec23<KT>(Ws, off, h, hf, t, r, ha, hb, o);
#pragma unroll
        for (int c = 0; c < 4; ++c) out[(8 * hf + 2 * c + t) * 64] = real ? o[c] : z;
    } else {
        const uint32_t off = (uint32_t)n * CP;
        const KQHead h     = kq_head45(Ws + off);
        const int gq       = wave;
        float d1lo, m1lo, d1hi, m1hi;
        kq_scale45(h, 2 * gq, d1lo, m1lo);
        kq_scale45(h, 2 * gq + 1, d1hi, m1hi);
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int r = 2 * rr + hi;
            uint32_t ha = 0, hb = 0;
            if (KT == 5) kq_ld8<true>(Ws, off + KQ<KT>::QH + 8 * r, ha, hb);
            half8_t lo, up;
            kq_dec45<KT>(Ws, off, gq, r, ha, hb, d1lo, m1lo, d1hi, m1hi, lo, up);
            out[(4 * gq + rr) * 64]     = real ? lo : z;  // weights 64 g + 16 rr + 8 hi + i
            out[(4 * gq + 2 + rr) * 64] = real ? up : z;  // weights 64 g + 32 + 16 rr + 8 hi + i
        }
    }
}

// =====================================================================================================
// launchers
// =====================================================================================================
static std::atomic<int64_t> g_kq_route_launches[KQ_ROUTE_COUNT];
int64_t kq_route_launches(int route) { return route >= 0 && route < KQ_ROUTE_COUNT ? g_kq_route_launches[route].load(std::memory_order_relaxed) : 0; }
static void kq_route_taken(KQRoute r) { g_kq_route_launches[r].fetch_add(1, std::memory_order_relaxed); }

bool kq_type(int wtype) { return wtype >= 10 && wtype <= 14; }
static int64_t kq_block_bytes(int wtype) { return wtype == 10 ? 84 : wtype == 11 ? 110 : wtype == 12 ? 144 : wtype == 13 ? 176 : 210; }
static bool kq_rows_aligned16(int wtype) { return wtype == 12 || wtype == 13; }

// The row range is k_qgemv's and k_qgemm16's together (options qgemm16_max_rows / qgemm16_rb are shared with k_qgemm16); the hand-over to the image route is
// set by profiles/kquant_probe.txt (one Linear, weights cache-warm, us):    4096 -> 3072 at 256 / 512 rows      3072 -> 9216 at 256 / 512 rows
//   q4_K  k_kq_gemm (64-row tiles)                                               56.1 / 75.0                         67.4 /  99.7
//   q4_0  k_qgemm16, parent commit                                               57.2 / 71.0                         81.0 /  80.5
//   q6_K  k_kq_gemm                                                              62.9 / 88.5                         89.1 / 134.2
//   q8_0  k_qgemm16, parent commit                                               60.8 / 75.9                         85.1 /  92.5
// q4_K keeps q4_0's range (option qgemm16_max_rows, 512): on a par with it, and the same argument holds (inside a model the weights arrive cold and the raw
// stream is 3.6x smaller than the image; the cache-warm image route measures 34 .. 64 us for every type).  q6_K is on a par with q8_0 up to 256 rows and 1.2 ..
// 1.5x slower at 512 (its decode reads three byte runs through v_alignbit per four fragments): it hands over at HALF the option, 256 rows.  q5_K (not probed:
// q4_K's decode plus one bit plane) takes q4_K's range.
// q2_K / q3_K against q4_K from the same run (profiles/kquant_low_probe.txt), k_kq_gemm at 512 rows, median [min .. max]:
//   q4_K   75.0 [74.5 .. 80.7]       100.8 [100.5 .. 100.9]
//   q2_K   74.0 [73.9 .. 77.1]        99.6 [ 99.6 ..  99.7]      no slower: the full range
//   q3_K   82.8 [80.3 .. 99.5]       113.4 [113.1 .. 115.4]      13 us slower on 3072 -> 9216 where the spreads are 0.4 .. 2.3 us (unaligned 8-byte reads
//                                                                  and the hmask plane per four fragments): half the option, 256 rows, as q6_K
bool kq_gemm_supported(int wtype, int64_t rows, int64_t K, int64_t M) {
    const int64_t max_rows = (wtype == 14 || wtype == 11) ? qgemm16_max_rows() / 2 : qgemm16_max_rows();
    return kq_type(wtype) && rows >= 1 && rows <= max_rows && K % 256 == 0 && K >= 256 && M >= 1 && M < (1ll << 30);
}
bool kq_image_supported(int wtype, int64_t K) { return kq_type(wtype) && K % 256 == 0 && K >= 256; }

// The grid of a launch, tile height and K slices together (the slices are counted on the tiles that are launched).
//   RB     32-row blocks per workgroup: 1 up to 32 rows, else 2; option qgemm16_rb = 1 / 2 / 4 forces that above 32 rows.  128-row tiles (RB 4: 86 .. 96 KB of
//          LDS and ~340 registers, one workgroup per CU) measured SLOWER than 64-row tiles on every probed shape, 256 rows to 4608 (q4_K 4096 -> 3072 at 512 rows
//          90.6 vs 75.0 us, 3072 -> 12288 at 4608 rows 870 vs 839 us; profiles/kquant_probe.txt): the default never takes them.
//   Split-K.  A launch of T = row tiles x ceil(M / 128) workgroups streams its weights at the HBM rate only with about two workgroups on each of the 256 CUs
//          (one is one wave per SIMD walking fetch -> LDS -> decode -> MFMA; a second hides that chain): S = 512 / T slices, each at least two segments long
//          (so that the prefetch overlaps something), at most 16.  FLUX modulation 3072 -> 18432 at 1 or 2 rows: T = 144, S = 3 -> 432 workgroups of 4 segments.
//          can_split = false (gated / GELU epilogues): S = 1.
static void kq_gemm_grid(int64_t rows, int64_t K, int64_t M, bool can_split, int& rb, int& S) {
    const int opt = qgemm16_rb();
    rb            = rows <= 32 ? 1 : 2;
    if (opt == 1 || opt == 2 || opt == 4) rb = rows <= 32 ? 1 : (rows <= 64 && opt > 2) ? 2 : opt;
    auto tiles  = [&](int b) { return ((rows + 32 * b - 1) / (32 * b)) * ((M + 127) / 128); };
    auto slices = [&](int64_t t) {
        int64_t n = can_split ? std::min<int64_t>(std::min<int64_t>(512 / t, K / 256 / 2), 16) : 1;
        return n < 2 ? 1 : (int)n;
    };
    S = slices(tiles(rb));
}
int kq_gemm_split_k(int64_t rows, int64_t K, int64_t M) {
    int rb, S;
    kq_gemm_grid(rows, K, M, true, rb, S);
    return S;
}

void launch_kq_gemm(hipStream_t s, float* dst, void* dst16, int64_t ldd16, const void* a16, int64_t lda, int64_t rows, const void* wraw, int wtype, int64_t K, int64_t M,
                    const Epilogue& ep, float* splitk_ws, int splitk_S, const float* x32, int64_t xs, float pre_scale, bool pre_silu) {
    if (!kq_gemm_supported(wtype, rows, K, M) || (a16 == nullptr) == (x32 == nullptr) || (ep.gelu && !dst16) || (!ep.gelu && !dst) || (ep.gate && !ep.residual) ||
        (kq_rows_aligned16(wtype) && ((uintptr_t)wraw & 15))) {
        fprintf(stderr, "ggml-mi355x: invalid k_kq_gemm request\n");
        abort();
    }
    const int64_t rowb = K / 256 * kq_block_bytes(wtype);
    KScope ks_(s, KF_QGEMM, 2.0 * rows * K * M, (double)M * rowb + (double)rows * K * (a16 ? 2.0 : 4.0) + (double)rows * M * 4.0);
    KQArgs g{};
    g.W = (const char*)wraw;
    g.row_bytes = rowb;
    g.A = (const _Float16*)a16; g.lda = lda;
    g.x32 = x32; g.xs = xs; g.pre_scale = pre_scale; g.pre_silu = pre_silu ? 1 : 0;
    g.dst = dst; g.ldd = M; g.dst16 = (_Float16*)dst16; g.ldd16 = ldd16;
    g.bias = ep.bias; g.residual = ep.residual; g.gate = ep.gate; g.gate_L = ep.gate_L > 0 ? ep.gate_L : 1; g.gelu = ep.gelu; g.scale = ep.scale;
    g.R = (int)rows; g.M = (int)M;
    if (ep.a_run_L > 0 && ep.a_run_S != ep.a_run_L) {
        g.a_runL = (int)ep.a_run_L;
        g.a_runS = (int)ep.a_run_S;
    }
    g.nseg = (int)(K / 256);
    const bool can_split = splitk_ws && splitk_S > 1 && !ep.gate && !ep.gelu && dst;
    int rb, S;
    kq_gemm_grid(rows, K, M, can_split, rb, S);
    if (can_split && S != splitk_S) {  // the planner sized the workspace with kq_gemm_split_k: same function, same answer
        fprintf(stderr, "ggml-mi355x: k_kq_gemm launched with %d K slices where its rule gives %d\n", splitk_S, S);
        abort();
    }
    g.nseg_slice = (g.nseg + S - 1) / S;
    if (S > 1) {
        g.slab = rows * M;
        g.dst  = splitk_ws;
    }
    const dim3 grid((unsigned)((rows + rb * 32 - 1) / (rb * 32)), (unsigned)((M + 127) / 128), (unsigned)S);
    kq_route_taken(rb == 1 ? KQ_GEMM_RB1 : rb == 2 ? KQ_GEMM_RB2 : KQ_GEMM_RB4);
#define KQ_LAUNCH(KT_)                                        \
    do {                                                      \
        if (rb == 1) k_kq_gemm<KT_, 1><<<grid, 256, 0, s>>>(g); \
        else if (rb == 2) k_kq_gemm<KT_, 2><<<grid, 256, 0, s>>>(g); \
        else k_kq_gemm<KT_, 4><<<grid, 256, 0, s>>>(g);       \
    } while (0)
    if (wtype == 10) KQ_LAUNCH(2);
    else if (wtype == 11) KQ_LAUNCH(3);
    else if (wtype == 12) KQ_LAUNCH(4);
    else if (wtype == 13) KQ_LAUNCH(5);
    else KQ_LAUNCH(6);
#undef KQ_LAUNCH
    if (S > 1) {
        kq_route_taken(KQ_GEMM_REDUCE);
        splitk_reduce_rows(s, dst, splitk_ws, S, rows * M, ep.bias, M, ep.residual);
    }
}

// k_kq_gemv: 1 .. 4 rows (option qgemv_max_rows), R x K halfs of staged rows within 48 KB (R = 1, 2, 4), whole super-blocks.  Every type ships: by the HIP-event
// sums its grouped launch beat the parent commit's separate k_kq_gemm launches on every probed shape (profiles/kq_gemv_probe.txt; by the host
// clock q3_K does not gain on the 3072-wide groups and loses 5 % on one of them).
bool kq_gemv_supported(int wtype, int64_t rows, int64_t K) {
    if (!kq_type(wtype) || rows < 1 || rows > std::min(4, qgemv_max_rows()) || K % 256 != 0 || K < 256) return false;
    return (rows <= 2 ? rows : 4) * K * 2 <= 48 * 1024;
}
static void kq_gemv_run(hipStream_t s, QGArgs& g, int wtype, int64_t rows, int64_t K, int64_t M) {
    if (!kq_gemv_supported(wtype, rows, K) || M < 1 || M >= (1ll << 31) || (!g.members && kq_rows_aligned16(wtype) && ((uintptr_t)g.W & 15))) {
        fprintf(stderr, "ggml-mi355x: invalid k_kq_gemv request\n");
        abort();
    }
    g.row_bytes = K / 256 * kq_block_bytes(wtype);
    g.K = (int)K; g.M = (int)M; g.rows = (int)rows;
    KScope ks_(s, KF_QGEMM, 2.0 * rows * K * M, (double)M * g.row_bytes + (double)rows * K * 4.0 + (double)rows * M * 4.0);
    KQVArgs a{g, (int)std::min<int64_t>(4, std::max<int64_t>(1, M / (16 * 1024)))};
    const unsigned grid = (unsigned)((M + 16 * a.gpw - 1) / (16 * a.gpw));
    const int r         = rows <= 2 ? (int)rows : 4;
    const size_t lds    = (size_t)r * K * 2;
    kq_route_taken(KQ_GEMV);
#define KQV_LAUNCH(KT_)                                              \
    do {                                                             \
        if (r == 1) k_kq_gemv<KT_, 1><<<grid, 256, lds, s>>>(a);      \
        else if (r == 2) k_kq_gemv<KT_, 2><<<grid, 256, lds, s>>>(a); \
        else k_kq_gemv<KT_, 4><<<grid, 256, lds, s>>>(a);             \
    } while (0)
    if (wtype == 10) KQV_LAUNCH(2);
    else if (wtype == 11) KQV_LAUNCH(3);
    else if (wtype == 12) KQV_LAUNCH(4);
    else if (wtype == 13) KQV_LAUNCH(5);
    else KQV_LAUNCH(6);
#undef KQV_LAUNCH
}
// x: f32 rows (stride xs floats, 16-byte aligned), staged as f16(silu?(x) * pre_scale); ep: scale, bias, residual (launch_qgemv's epilogue)
void launch_kq_gemv(hipStream_t s, float* dst, int64_t ldd, const float* x, int64_t xs, int64_t rows, const void* wraw, int wtype, int64_t K, int64_t M, const Epilogue& ep,
                    float pre_scale, bool pre_silu) {
    if (ep.gate || ep.gelu) {
        fprintf(stderr, "ggml-mi355x: k_kq_gemv has no gate / GELU epilogue\n");
        abort();
    }
    QGArgs g;
    g.W = (const char*)wraw;
    g.x = x; g.xs = xs;
    g.dst = dst; g.ldd = ldd;
    g.bias = ep.bias; g.residual = ep.residual; g.scale = ep.scale; g.pre_scale = pre_scale; g.pre_silu = pre_silu ? 1 : 0;
    kq_gemv_run(s, g, wtype, rows, K, M);
}
// the grouped form of launch_qgemv_group (same member table: qgemv_fill_member; every member a multiple of 4 rows, q4_K / q5_K members 16-byte aligned)
void launch_kq_gemv_group(hipStream_t s, float* dst, int64_t Mtot, const float* x, int64_t xs, int64_t rows, const void* members_dev, int n_members, int wtype, int64_t K,
                          float pre_scale, bool pre_silu) {
    // the table lives in device memory: only the sum of the members' sizes can be checked here; each member being a multiple of 4 rows (a wave's four rows come
    // from ONE base pointer) and 16-byte aligned for q4_K / q5_K is the caller's contract (kernels.h; plan_hoisted_mod enforces both)
    if (!members_dev || n_members < 1 || Mtot % KQV_CPW != 0) {
        fprintf(stderr, "ggml-mi355x: invalid k_kq_gemv group (%d members, %lld columns: every member must be a multiple of %d rows)\n", n_members, (long long)Mtot, KQV_CPW);
        abort();
    }
    QGArgs g;
    g.members   = (const QGMember*)members_dev;
    g.n_members = n_members;
    g.W         = nullptr;
    g.x = x; g.xs = xs;
    g.dst = dst; g.ldd = Mtot;
    g.bias = nullptr; g.residual = nullptr; g.scale = 1.f; g.pre_scale = pre_scale; g.pre_silu = pre_silu ? 1 : 0;
    kq_gemv_run(s, g, wtype, rows, K, Mtot);
}

// dst: image of wswz_bytes(R, K) bytes (rows padded to 128); geglu_inner as launch_wswz_linear takes it
void launch_kq_image(hipStream_t s, void* dst, const void* wraw, int wtype, int64_t K, int64_t R, int64_t geglu_inner) {
    if (!kq_image_supported(wtype, K) || R < 1 || (kq_rows_aligned16(wtype) && ((uintptr_t)wraw & 15))) {
        fprintf(stderr, "ggml-mi355x: invalid k_kq_image request\n");
        abort();
    }
    const int64_t Rp = (R + 127) / 128 * 128, rowb = K / 256 * kq_block_bytes(wtype);
    KScope ks_(s, KF_PACK_F16, 0.0, (double)R * rowb + (double)Rp * K * 2.0);
    const dim3 grid((unsigned)(Rp / 32), (unsigned)(K / 256));
    kq_route_taken(KQ_IMAGE);
    if (wtype == 10) k_kq_image<2><<<grid, 256, 0, s>>>((half8_t*)dst, (const char*)wraw, rowb, R, K / 16, geglu_inner);
    else if (wtype == 11) k_kq_image<3><<<grid, 256, 0, s>>>((half8_t*)dst, (const char*)wraw, rowb, R, K / 16, geglu_inner);
    else if (wtype == 12) k_kq_image<4><<<grid, 256, 0, s>>>((half8_t*)dst, (const char*)wraw, rowb, R, K / 16, geglu_inner);
    else if (wtype == 13) k_kq_image<5><<<grid, 256, 0, s>>>((half8_t*)dst, (const char*)wraw, rowb, R, K / 16, geglu_inner);
    else k_kq_image<6><<<grid, 256, 0, s>>>((half8_t*)dst, (const char*)wraw, rowb, R, K / 16, geglu_inner);
}

}  // namespace mi355x
