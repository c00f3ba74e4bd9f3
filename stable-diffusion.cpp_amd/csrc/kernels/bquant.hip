// bquant.hip — Linear layers whose weights are the 32-weight GGUF blocks q4_1 / q5_0 / q5_1 / iq4_nl (what --type q4_1 / q5_0 / q5_1 writes, and what ggml's
// quantiser falls back to inside a K-quant file for every row length that is no multiple of 256: the 320- and 640-wide Linears of the SD1.5 / SDXL UNets), kept RAW
// in HBM (0.625 / 0.6875 / 0.75 / 0.5625 B per weight).
//
// ONE weight value on every route: w16 = f16(y), y = the f32 value of ggml's dequantize_row_*:
//   q4_1   {f16 d, f16 m, u8 qs[16]}            20 B   y = q * d + m
//   q5_0   {f16 d, u8 qh[4], u8 qs[16]}         22 B   y = (q - 16) * d
//   q5_1   {f16 d, f16 m, u8 qh[4], u8 qs[16]}  24 B   y = q * d + m
//   iq4_nl {f16 d, u8 qs[16]}                   18 B   y = d * kvalues[q]      (ggml's 16-entry table -127 .. 113)
//   mxfp4  {u8 e, u8 qs[16]}                    17 B   y = kvalues[q] * 2^(e - 128)   (the e2m1 values doubled; rows at ANY byte phase: BQ<39>, BQStrip<39>,
//                                                      bq_block<39> below and mxfp4_decode.h)
// element j of a block: low nibble of qs[j], element j + 16: high nibble; fifth bit = bit j / j + 16 of the little-endian u32 qh.
// Every product is EXACT in f32 (an integer of at most 7 bits times an f16 of 11), so y carries at most one f32 rounding, the "+ m": fused or unfused evaluation
// give the same y, and bit equality with a NumPy float32 restatement is well defined.  f32 -> f16 is a SECOND rounding and stays one: y is formed with plain f32
// operators under fp contract(off) (never a v_fma_mix that rounds q * d + m straight to f16; the compiler does emit v_fma_mixlo_f16 with a ZERO addend for the
// one-product types q5_0 / iq4_nl, which is f16 of the exact product, the same value) and then converted.  The few-row kernel and the image kernel share
// the decoder (bq_block), so a Linear differs between its routes by f32 summation order only.
//
//   k_bq_gemm<BT, RB>   1 .. bq max rows activation rows: the raw blocks stream from HBM once and are decoded in registers into the f16 B fragments of
//                       v_mfma_f32_32x32x16_f16; no image exists.  Tile 32 RB rows x 128 columns, 4 waves x 32 columns, lane = (column n = lane % 32, k half
//                       kg = lane / 32).  A K segment is up to 8 blocks (256 weights) of each of the wave's 32 columns; the last one is shorter when K % 256 != 0.
//                       Per block the lane reads qs[8 kg .. 8 kg + 7]: their low nibbles are weights 8 kg + i (the block's first MFMA step), their high nibbles
//                       weights 16 + 8 kg + i (the second): k runs in natural order, the A fragments are read unpermuted, no lane shuffles.  The fifth bits of
//                       those eight weights are byte kg / byte 2 + kg of qh, spread to bit 4 of eight bytes by one multiply per four (x * 0x00204081 & 0x01010101).
//                       iq4_nl: the table lives in four registers; four nibbles are looked up at once by two v_perm_b32 (entries 0 .. 7 / 8 .. 15, selector =
//                       nibble & 7) and a bit select on nibble bit 3 — no branch, no memory.
//                       Rows are 2- (q5_0, iq4_nl), 4- (q4_1) or 8-byte (q5_1) aligned, never 16: per segment a wave fetches, for each of ITS 32 columns, the
//                       ALIGNED 16-byte granules that cover the column's piece — only those that hold a valid byte, so nothing outside the tensor's pages is touched —
//                       into a per-wave LDS strip, and the LDS reads re-align (v_alignbit for the 2-byte aligned types).
//                       Strip stride per column: 16 NGC + 8 bytes (NGC = covering granules of a full piece: 11 / 12 / 13 / 10) = 184 / 200 / 216 / 168.  The pieces
//                       themselves (160 / 176 / 192 / 144 B) and their granule multiples are 4 x even dwords apart: 32 columns would fall on 4 .. 16 of the 64 banks.
//                       The padded strides are 46 / 50 / 54 / 42 dwords, 2 x odd: the 32 columns start on 32 different even banks (the price: the stash is two
//                       8-byte LDS stores per granule instead of one of 16).
//                       The next segment's global loads are in flight during the MFMAs; split-K over gridDim.z into f32 slabs (splitk_reduce_rows).
//                       A = the f16 operand image, or for 1 .. 4 rows the f32 rows themselves (SiLU and pre_scale applied while they are staged).
//   k_bq_image<BT>      raw blocks -> the f16 fragment-order image [col/32][Kp/16][64 lanes][8 halfs] of k_gemm16 (Kp = K rounded up to 64, the pad zero; plain row
//                       order and both GEGLU orders of k_wswz_linear), any K % 32 == 0.  A workgroup owns 32 image rows x 256 k: it loads the row pieces coalesced into
//                       one LDS strip (same covering granules), wave w decodes blocks 2 w and 2 w + 1 — each lane its row's header once per block — and writes four
//                       whole 1 KiB fragments.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include "device_utils.h"
#include "kernels.h"
#include "ktime.h"
#include "mxfp4_decode.h"

namespace mi355x {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// BT = the ggml type id.  QH / QS: byte offsets of qh / qs in a block; A4: every field read is 4-byte aligned
template <int BT>
struct BQ;
template <>
struct BQ<3> {  // q4_1
    static constexpr int BS = 20, QH = -1, QS = 4;
    static constexpr bool HASM = true, A4 = true;
};
template <>
struct BQ<6> {  // q5_0
    static constexpr int BS = 22, QH = 2, QS = 6;
    static constexpr bool HASM = false, A4 = false;
};
template <>
struct BQ<7> {  // q5_1
    static constexpr int BS = 24, QH = 4, QS = 8;
    static constexpr bool HASM = true, A4 = true;
};
template <>
struct BQ<20> {  // iq4_nl
    static constexpr int BS = 18, QH = -1, QS = 2;
    static constexpr bool HASM = false, A4 = false;
};
template <>
struct BQ<39> {  // mxfp4: {u8 e, u8 qs[16]}, no f16 field; rows start at any byte
    static constexpr int BS = 17, QH = -1, QS = 1;
    static constexpr bool HASM = false, A4 = false;
};
// a full piece is 8 BS bytes at a phase of at most 14 (BS even): 8 BS / 16 + 1 aligned granules cover it
template <int BT>
struct BQStrip {
    static constexpr int NGC = BQ<BT>::BS / 2 + 1;
    static constexpr int CP  = 16 * NGC + 8;   // bytes between the columns of a strip: 2 x odd dwords (file header)
    static constexpr int NGW = 32 * NGC;       // granules of a 32-column strip
    static constexpr int BYTES = 32 * CP + 16; // (+ 16: the third dword of an unaligned 8-byte read at the strip's end)
};

// mxfp4: a full piece is 136 bytes at a phase of 0 .. 15: ceil((15 + 136) / 16) = 10 aligned granules cover it.  Stride 168 bytes = 42 dwords = 2 x 21: column n
// starts on bank 42 n mod 64, 32 different even banks (21 is odd).  The farthest read, the third dword of block 7's upper code half at phase 15, ends at byte
// 152 of its column.
template <>
struct BQStrip<39> {
    static constexpr int NGC = 10;
    static constexpr int CP  = 16 * NGC + 8;
    static constexpr int NGW = 32 * NGC;
    static constexpr int BYTES = 32 * CP + 16;
};

constexpr int8_t kIQ4NL[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113};
constexpr uint32_t iq4_word(int i) {
    return (uint32_t)(uint8_t)kIQ4NL[4 * i] | ((uint32_t)(uint8_t)kIQ4NL[4 * i + 1] << 8) | ((uint32_t)(uint8_t)kIQ4NL[4 * i + 2] << 16) | ((uint32_t)(uint8_t)kIQ4NL[4 * i + 3] << 24);
}
constexpr uint32_t kIQ4W0 = iq4_word(0), kIQ4W1 = iq4_word(1), kIQ4W2 = iq4_word(2), kIQ4W3 = iq4_word(3);
// four nibbles (one per byte of q) -> their four table entries (int8, one per byte).  v_perm_b32 takes selector bytes 0 .. 3 from its second operand, 4 .. 7 from its first
__device__ __forceinline__ uint32_t iq4_lookup4(uint32_t q) {
    const uint32_t sel = q & 0x07070707u;
    const uint32_t lo  = __builtin_amdgcn_perm(kIQ4W1, kIQ4W0, sel);
    const uint32_t hi  = __builtin_amdgcn_perm(kIQ4W3, kIQ4W2, sel);
    const uint32_t msk = ((q >> 3) & 0x01010101u) * 0xFFu;
    return (hi & msk) | (lo & ~msk);
}
// bit i of the low four bits of x -> bit 4 of byte i (x * 0x00204081 puts bit i at 8 i: the four shifted copies never meet)
__device__ __forceinline__ uint32_t bq_fifth(uint32_t x) { return (((x & 0xFu) * 0x00204081u) & 0x01010101u) << 4; }

// 8 bytes at byte offset off of an LDS strip: 4-byte aligned, or 2-byte aligned through three dwords and v_alignbit
template <bool A4>
__device__ __forceinline__ void bq_ld8(const char* strip, uint32_t off, uint32_t& a, uint32_t& b) {
    if (A4) {
        a = *(const uint32_t*)(strip + off);
        b = *(const uint32_t*)(strip + off + 4);
    } else {
        const char* p     = strip + (off & ~3u);
        const uint32_t sh = (off & 2u) * 8u;
        const uint32_t r0 = *(const uint32_t*)p, r1 = *(const uint32_t*)(p + 4), r2 = *(const uint32_t*)(p + 8);
        a = __builtin_amdgcn_alignbit(r1, r0, sh);
        b = __builtin_amdgcn_alignbit(r2, r1, sh);
    }
}

// eight codes (one per byte of a, b) -> f16(y); each f32 operation rounded on its own, the conversion a rounding of its own
template <int BT>
__device__ __forceinline__ half8_t bq_w8(uint32_t a, uint32_t b, float d, float m) {
#pragma clang fp contract(off)  // plain operators under this pragma: the product and the sum are never one v_fma_mix that rounds straight to f16
    half8_t o;
    if (BT == 20) {
        a = iq4_lookup4(a);
        b = iq4_lookup4(b);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (BT == 20) {
            o[j]     = (_Float16)(d * (float)(int)(int8_t)(a >> (8 * j)));
            o[4 + j] = (_Float16)(d * (float)(int)(int8_t)(b >> (8 * j)));
        } else if (BT == 6) {
            o[j]     = (_Float16)((float)((int)((a >> (8 * j)) & 0xFFu) - 16) * d);
            o[4 + j] = (_Float16)((float)((int)((b >> (8 * j)) & 0xFFu) - 16) * d);
        } else {
            const float pa = (float)((a >> (8 * j)) & 0xFFu) * d, pb = (float)((b >> (8 * j)) & 0xFFu) * d;
            o[j]     = (_Float16)(pa + m);
            o[4 + j] = (_Float16)(pb + m);
        }
    }
    return o;
}

// the block at strip + off (off of the block's alignment), k half kg: lo = weights 8 kg + i, hi = weights 16 + 8 kg + i
template <int BT>
__device__ __forceinline__ void bq_block(const char* strip, uint32_t off, int kg, half8_t& lo, half8_t& hi) {
    const float d = (float)*(const _Float16*)(strip + off);
    const float m = BQ<BT>::HASM ? (float)*(const _Float16*)(strip + off + 2) : 0.f;
    uint32_t a, b;
    bq_ld8<BQ<BT>::A4>(strip, off + BQ<BT>::QS + 8 * kg, a, b);
    uint32_t la = a & 0x0F0F0F0Fu, lb = b & 0x0F0F0F0Fu, ua = (a >> 4) & 0x0F0F0F0Fu, ub = (b >> 4) & 0x0F0F0F0Fu;
    if (BQ<BT>::QH >= 0) {  // byte kg of qh: fifth bits of weights 8 kg + i; byte 2 + kg: of weights 16 + 8 kg + i
        const uint32_t h0 = *(const uint8_t*)(strip + off + BQ<BT>::QH + kg), h1 = *(const uint8_t*)(strip + off + BQ<BT>::QH + 2 + kg);
        la |= bq_fifth(h0);
        lb |= bq_fifth(h0 >> 4);
        ua |= bq_fifth(h1);
        ub |= bq_fifth(h1 >> 4);
    }
    lo = bq_w8<BT>(la, lb, d, m);
    hi = bq_w8<BT>(ua, ub, d, m);
}

// mxfp4: the exponent byte gives the block's table registers and f16 scale (mxfp4_decode.h); the eight code bytes lie at ANY byte offset: three dwords and
// v_alignbit by 0 / 8 / 16 / 24 bits.  Four codes -> two half2, in k order
template <>
__device__ __forceinline__ void bq_block<39>(const char* strip, uint32_t off, int kg, half8_t& lo, half8_t& hi) {
    const MX4Scale m  = mx4_prep(*(const uint8_t*)(strip + off));
    const uint32_t o  = off + 1 + 8 * kg;
    const char* p     = strip + (o & ~3u);
    const uint32_t sh = (o & 3u) * 8u;
    const uint32_t r0 = *(const uint32_t*)p, r1 = *(const uint32_t*)(p + 4), r2 = *(const uint32_t*)(p + 8);
    const uint32_t a = __builtin_amdgcn_alignbit(r1, r0, sh), b = __builtin_amdgcn_alignbit(r2, r1, sh);
    mx4_half2_t l[4], u[4];
    mx4_w4(a & 0x0F0F0F0Fu, m, l[0], l[1]);
    mx4_w4(b & 0x0F0F0F0Fu, m, l[2], l[3]);
    mx4_w4((a >> 4) & 0x0F0F0F0Fu, m, u[0], u[1]);
    mx4_w4((b >> 4) & 0x0F0F0F0Fu, m, u[2], u[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        lo[2 * j] = l[j][0], lo[2 * j + 1] = l[j][1];
        hi[2 * j] = u[j][0], hi[2 * j + 1] = u[j][1];
    }
}

// granule gr of the covering fetch of the nb-block piece at p: loaded only if it holds a valid byte (else zero, never read as a weight)
template <int BT>
__device__ __forceinline__ u32x4_t bq_fetch(const char* p, int gr, int nb) {
    const uint32_t ph = (uint32_t)((uintptr_t)p & 15);
    u32x4_t v         = {0, 0, 0, 0};
    if ((uint32_t)gr * 16u < ph + (uint32_t)nb * BQ<BT>::BS) v = *(const u32x4_t*)(p - ph + gr * 16);
    return v;
}
__device__ __forceinline__ void bq_stash(char* strip, int cp, int col, int gr, const u32x4_t& v) {  // the stride is a multiple of 8, not of 16
    uint2* q = (uint2*)(strip + col * cp + gr * 16);
    q[0]     = make_uint2(v[0], v[1]);
    q[1]     = make_uint2(v[2], v[3]);
}

// =====================================================================================================
// k_bq_gemm
// =====================================================================================================
struct BQArgs {
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
    int KB;  // blocks per row
    int nseg, nseg_slice;
    int64_t slab;
    int a_runL, a_runS;
};

template <int BT, int RB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_bq_gemm(BQArgs g) {  // two workgroups per CU: at most 256 registers (q5_1 on 64-row tiles took 260 without the bound)
    constexpr int BS  = BQ<BT>::BS;
    constexpr int NGC = BQStrip<BT>::NGC;
    constexpr int CP  = BQStrip<BT>::CP;
    constexpr int NGW = BQStrip<BT>::NGW;
    constexpr int NLW = (NGW + 63) / 64;   // loads per lane: 6 / 6 / 7 / 5
    constexpr int RT  = RB * 32;
    constexpr int AS  = 256 * 2 + 16;      // bytes between A rows in LDS
    constexpr int NLA = RT * 32 / 256;     // A granules per thread
    __shared__ __attribute__((aligned(16))) char As[RT * AS];
    __shared__ __attribute__((aligned(16))) char Wsm[4][BQStrip<BT>::BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 31, kg = lane >> 5;
    char* Ws           = Wsm[wave];
    const int64_t row0 = (int64_t)blockIdx.x * RT;
    const int colw     = (int)blockIdx.y * 128 + wave * 32;
    const int seg0     = (int)blockIdx.z * g.nseg_slice;
    const int seg1     = min(g.nseg, seg0 + g.nseg_slice);
    const char* mycol  = g.W + (int64_t)min(colw + n, g.M - 1) * g.row_bytes;  // this lane's column: its phase inside the strip

    float16_t acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[rb][i] = 0.f;

    u32x4_t wreg[NLW], areg[NLA];
    auto a_phys = [&](int64_t r) -> int64_t {
        return g.a_runL > 0 ? (int64_t)((uint32_t)r / (uint32_t)g.a_runL) * g.a_runS + (uint32_t)r % (uint32_t)g.a_runL : r;
    };
    auto blocks_of = [&](int seg) { return min(8, g.KB - seg * 8); };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < NLW; ++i) {
            const int idx = i * 64 + lane;
            if (idx < NGW) bq_stash(Ws, CP, idx / NGC, idx % NGC, wreg[i]);
        }
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int idx = i * 256 + (int)threadIdx.x;
            *(u32x4_t*)(As + (idx >> 5) * AS + (idx & 31) * 16) = areg[i];
        }
    };
    auto fetch = [&](int seg) {
        const int nb = blocks_of(seg);
#pragma unroll
        for (int i = 0; i < NLW; ++i) {
            const int idx = i * 64 + lane;
            const int col = idx / NGC, gr = idx - col * NGC;
            const int cc  = min(colw + col, g.M - 1);
            wreg[i]       = (u32x4_t){0, 0, 0, 0};
            if (idx < NGW) wreg[i] = bq_fetch<BT>(g.W + (int64_t)cc * g.row_bytes + (int64_t)seg * (8 * BS), gr, nb);
        }
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int idx     = i * 256 + (int)threadIdx.x;
            const int row     = idx >> 5, gr = idx & 31;
            const int64_t grw = row0 + row;
            areg[i]           = (u32x4_t){0, 0, 0, 0};
            if (grw < g.R && gr * 8 < nb * 32) {  // (a short last segment: nothing is read beyond k = K)
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
        const int nb       = blocks_of(seg);  // workgroup-uniform
        const uint32_t off = (uint32_t)n * CP + (uint32_t)((uintptr_t)(mycol + (int64_t)seg * (8 * BS)) & 15);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            if (b >= nb) break;
            half8_t lo, hi;
            bq_block<BT>(Ws, off + b * BS, kg, lo, hi);
            step(lo, 32 * b + 8 * kg);
            step(hi, 32 * b + 16 + 8 * kg);
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
// k_bq_image
// =====================================================================================================
// source row of image row (32-row block rb, n) under k_wswz_linear's three orders; >= R: a zero row
__device__ __forceinline__ int64_t bq_image_row(int64_t rb, int n, int64_t R, int64_t geglu_inner) {
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

// grid (image rows / 32, ceil(Kp / 256)); KB = K / 32 blocks per row, kfr = Kp / 16 fragments per 32-row block
template <int BT>
__global__ __launch_bounds__(256) void k_bq_image(half8_t* __restrict__ dst, const char* __restrict__ W, int64_t row_bytes, int64_t R, int KB, int64_t kfr, int64_t geglu_inner) {
    constexpr int BS  = BQ<BT>::BS;
    constexpr int NGC = BQStrip<BT>::NGC;
    constexpr int CP  = BQStrip<BT>::CP;
    constexpr int NGW = BQStrip<BT>::NGW;
    __shared__ __attribute__((aligned(16))) char Ws[BQStrip<BT>::BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lane & 31, hi = lane >> 5;
    const int64_t rb = blockIdx.x;
    const int seg    = blockIdx.y;
    const int nb     = min(8, KB - seg * 8);                     // blocks of this segment (>= 1)
    const int nfr    = (int)min((int64_t)16, kfr - seg * 16);    // fragments of this segment: 2 nb, or 2 nb + 2 with the zero pad up to Kp
    for (int idx = threadIdx.x; idx < NGW; idx += 256) {
        const int col    = idx / NGC, gr = idx - col * NGC;
        const int64_t rr = min(bq_image_row(rb, col, R, geglu_inner), R - 1);
        bq_stash(Ws, CP, col, gr, bq_fetch<BT>(W + rr * row_bytes + (int64_t)seg * (8 * BS), gr, nb));
    }
    __syncthreads();
    const int64_t src  = bq_image_row(rb, n, R, geglu_inner);
    const bool real    = src < R;
    half8_t* out       = dst + (rb * kfr + (int64_t)seg * 16) * 64 + lane;
    const half8_t z    = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t off = (uint32_t)n * CP + (uint32_t)((uintptr_t)(W + min(src, R - 1) * row_bytes + (int64_t)seg * (8 * BS)) & 15);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int b = 2 * wave + t;  // wave-uniform
        if (2 * b >= nfr) break;
        half8_t lo = z, up = z;
        if (b < nb) bq_block<BT>(Ws, off + b * BS, hi, lo, up);
        out[(2 * b) * 64]     = real ? lo : z;  // weights 32 b + 8 hi + i
        out[(2 * b + 1) * 64] = real ? up : z;  // weights 32 b + 16 + 8 hi + i
    }
}

// =====================================================================================================
// launchers
// =====================================================================================================
static std::atomic<int64_t> g_bq_route_launches[BQ_ROUTE_COUNT];
int64_t bq_route_launches(int route) { return route >= 0 && route < BQ_ROUTE_COUNT ? g_bq_route_launches[route].load(std::memory_order_relaxed) : 0; }
static void bq_route_taken(BQRoute r) { g_bq_route_launches[r].fetch_add(1, std::memory_order_relaxed); }

bool bq_type(int wtype) { return wtype == 3 || wtype == 6 || wtype == 7 || wtype == 20 || wtype == 39; }
static int64_t bq_block_bytes(int wtype) { return wtype == 3 ? 20 : wtype == 6 ? 22 : wtype == 7 ? 24 : wtype == 39 ? 17 : 18; }

// The row range is shared with k_qgemm16 and k_kq_gemm (option qgemm16_max_rows, 512), one value for the five types (mxfp4: profiles/mxfp4_probe.txt, at or below iq4_nl at every row count).  profiles/bquant_probe.txt (one Linear,
// weights cache-warm, us) does NOT show the kernel ahead of its own cached-image route: 4096 -> 3072 at 256 / 512 rows 58 / 78 (q5_0 60 / 84) against 34 / 45,
// 1280 -> 1280 at 1 row 29 against 20; a tie at 768 -> 320 and at 3072 -> 18432, 1 row.  q4_0's k_qgemm16 (parent commit: 56.7 / 70.0) loses to its image alike;
// this kernel is 1.01 .. 1.12x of it (q5_0 1.06 .. 1.20x).  The range is kept for what it is kept for there: no f16 image (2 B per weight) exists for such a Linear.
int bq_gemm_max_rows(int wtype) {
    (void)wtype;
    return qgemm16_max_rows();
}
bool bq_gemm_supported(int wtype, int64_t rows, int64_t K, int64_t M) {
    return bq_type(wtype) && rows >= 1 && rows <= bq_gemm_max_rows(wtype) && K % 32 == 0 && K >= 32 && K < (1ll << 30) && M >= 1 && M < (1ll << 30);
}
bool bq_image_supported(int wtype, int64_t K) { return bq_type(wtype) && K % 32 == 0 && K >= 32 && K < (1ll << 30); }

// The grid of a launch, tile height and K slices together (k_kq_gemm's rule on this kernel's segments).
//   RB     32-row blocks per workgroup: 1 up to 32 rows, else 2 (option qgemm16_rb = 1 forces 32-row tiles).  k_kq_gemm measured 128-row tiles slower than 64-row
//          tiles on every shape; this kernel has none.
//   Split-K.  T = row tiles x ceil(M / 128) workgroups stream their weights at the HBM rate only with about two workgroups on each of the 256 CUs: S = 512 / T slices,
//          each at least two segments long (so that the prefetch overlaps something), at most 16.  nseg = ceil(K / 256): the smallest K that splits is 800 (4 segments,
//          the last of one block), on a grid of at most 256 tiles.  can_split = false (gated / GELU epilogues): S = 1.
static void bq_gemm_grid(int64_t rows, int64_t K, int64_t M, bool can_split, int& rb, int& S) {
    rb                  = (rows <= 32 || qgemm16_rb() == 1) ? 1 : 2;
    const int64_t t     = ((rows + 32 * rb - 1) / (32 * rb)) * ((M + 127) / 128);
    const int64_t nseg  = (K + 255) / 256;
    const int64_t n     = can_split ? std::min<int64_t>(std::min<int64_t>(512 / t, nseg / 2), 16) : 1;
    S                   = n < 2 ? 1 : (int)n;
}
int bq_gemm_split_k(int64_t rows, int64_t K, int64_t M) {
    int rb, S;
    bq_gemm_grid(rows, K, M, true, rb, S);
    return S;
}

void launch_bq_gemm(hipStream_t s, float* dst, void* dst16, int64_t ldd16, const void* a16, int64_t lda, int64_t rows, const void* wraw, int wtype, int64_t K, int64_t M,
                    const Epilogue& ep, float* splitk_ws, int splitk_S, const float* x32, int64_t xs, float pre_scale, bool pre_silu) {
    if (!bq_gemm_supported(wtype, rows, K, M) || (a16 == nullptr) == (x32 == nullptr) || (ep.gelu && !dst16) || (!ep.gelu && !dst) || (ep.gate && !ep.residual) ||
        ((uintptr_t)wraw & 15)) {
        fprintf(stderr, "ggml-mi355x: invalid k_bq_gemm request\n");
        abort();
    }
    const int64_t rowb = K / 32 * bq_block_bytes(wtype);
    KScope ks_(s, KF_QGEMM, 2.0 * rows * K * M, (double)M * rowb + (double)rows * K * (a16 ? 2.0 : 4.0) + (double)rows * M * 4.0);
    BQArgs g{};
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
    g.KB   = (int)(K / 32);
    g.nseg = (int)((K + 255) / 256);
    const bool can_split = splitk_ws && splitk_S > 1 && !ep.gate && !ep.gelu && dst;
    int rb, S;
    bq_gemm_grid(rows, K, M, can_split, rb, S);
    if (can_split && S != splitk_S) {  // the planner sized the workspace with bq_gemm_split_k: same function, same answer
        fprintf(stderr, "ggml-mi355x: k_bq_gemm launched with %d K slices where its rule gives %d\n", splitk_S, S);
        abort();
    }
    g.nseg_slice = (g.nseg + S - 1) / S;
    if (S > 1) {
        g.slab = rows * M;
        g.dst  = splitk_ws;
    }
    const dim3 grid((unsigned)((rows + rb * 32 - 1) / (rb * 32)), (unsigned)((M + 127) / 128), (unsigned)S);
    bq_route_taken(rb == 1 ? BQ_GEMM_RB1 : BQ_GEMM_RB2);
#define BQ_LAUNCH(BT_)                                          \
    do {                                                        \
        if (rb == 1) k_bq_gemm<BT_, 1><<<grid, 256, 0, s>>>(g); \
        else k_bq_gemm<BT_, 2><<<grid, 256, 0, s>>>(g);         \
    } while (0)
    if (wtype == 3) BQ_LAUNCH(3);
    else if (wtype == 6) BQ_LAUNCH(6);
    else if (wtype == 7) BQ_LAUNCH(7);
    else if (wtype == 39) BQ_LAUNCH(39);
    else BQ_LAUNCH(20);
#undef BQ_LAUNCH
    if (S > 1) {
        bq_route_taken(BQ_GEMM_REDUCE);
        splitk_reduce_rows(s, dst, splitk_ws, S, rows * M, ep.bias, M, ep.residual);
    }
}

// dst: image of wswz_bytes(R, K) bytes (rows padded to 128, K to 64); geglu_inner as launch_wswz_linear takes it
void launch_bq_image(hipStream_t s, void* dst, const void* wraw, int wtype, int64_t K, int64_t R, int64_t geglu_inner) {
    if (!bq_image_supported(wtype, K) || R < 1 || ((uintptr_t)wraw & 15)) {
        fprintf(stderr, "ggml-mi355x: invalid k_bq_image request\n");
        abort();
    }
    const int64_t Rp = (R + 127) / 128 * 128, Kp = (K + 63) / 64 * 64, rowb = K / 32 * bq_block_bytes(wtype);
    KScope ks_(s, KF_PACK_F16, 0.0, (double)R * rowb + (double)Rp * Kp * 2.0);
    const dim3 grid((unsigned)(Rp / 32), (unsigned)((Kp + 255) / 256));
    bq_route_taken(BQ_IMAGE);
    half8_t* d    = (half8_t*)dst;
    const char* w = (const char*)wraw;
    if (wtype == 3) k_bq_image<3><<<grid, 256, 0, s>>>(d, w, rowb, R, (int)(K / 32), Kp / 16, geglu_inner);
    else if (wtype == 6) k_bq_image<6><<<grid, 256, 0, s>>>(d, w, rowb, R, (int)(K / 32), Kp / 16, geglu_inner);
    else if (wtype == 7) k_bq_image<7><<<grid, 256, 0, s>>>(d, w, rowb, R, (int)(K / 32), Kp / 16, geglu_inner);
    else if (wtype == 39) k_bq_image<39><<<grid, 256, 0, s>>>(d, w, rowb, R, (int)(K / 32), Kp / 16, geglu_inner);
    else k_bq_image<20><<<grid, 256, 0, s>>>(d, w, rowb, R, (int)(K / 32), Kp / 16, geglu_inner);
}

}  // namespace mi355x
