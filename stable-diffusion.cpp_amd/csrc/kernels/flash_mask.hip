// flash_mask.hip — masked attention forward for gfx950: softmax(scale * Q K^T + M) V with online softmax, head dims 64 and 128, the scores never leave the CU.
// Reached through launch_flash_attn when the FLASH_ATTN_EXT node carries a mask (src[3]): the causal mask of the CLIP text towers (-inf above the diagonal), T5's
// per-head relative-position bias, key-padding masks.  Operands as ggml_ext_attention_ext emits them: Q f32 d-contiguous, K / V f16 d-contiguous with 16-byte
// aligned rows, M f16 [Lk, >= Lq, Hm, 1] contiguous (head hn reads plane hn % Hm; its rows are only 2-byte aligned: Lk = 77 gives 154-byte rows).
//
// Work split and K / V movement are k_flash_attn's select-free FAST form (flash_attn.hip): a workgroup = 4 waves x 32 query rows of one (head, image), 64-key tiles,
// K and V staged with 16-byte buffer loads, register-prefetched one tile ahead into two LDS tile buffers (one barrier per tile), S^T = K Q^T computed swapped so that
// a lane holds ONE query's scores for 32 keys (its l ^ 32 partner the other 32), P fed back as the A operand in the accumulator's own key order, V read with
// ds_read_b64_tr_b16 from the row-major tile.
//
// The mask is the new stream: 32 queries x 64 keys of f16 per wave and tile.  Each wave stages ITS OWN rows (nobody else reads them), so the stream needs no
// barrier of its own:
//   * global -> registers, one tile ahead of the LDS copy (two ahead of its use), coalesced along the key axis.  Lk % 4 == 0 and an 8-byte aligned tensor: 8-byte
//     loads, lane -> (row l >> 4 of a group of four rows, 4-key chunk l & 15), 8 per lane and tile.  Anything else (Lk = 77): 2-byte loads, lane -> key, one row per
//     instruction, 32 per lane and tile, packed into the same 16 registers.  Every load goes through a buffer descriptor of ONE mask plane with the whole offset in
//     the per-lane (range-checked) operand; elements outside the tile's real part — keys >= Lk of a ragged last tile, rows >= Lq — point beyond the descriptor,
//     fetch nothing, and are stored as -inf.  So a ragged key tail needs no masking code of its own, and no load reaches past its row.
//   * registers -> LDS [32 rows][68 halfs] per wave (136-byte rows: the 8-byte reads of 32 rows fall on distinct banks, as FA_VTS), ONE buffer: the copy of tile
//     t + 1 is written after the wave has read tile t, and the barrier that ends the tile orders it before the next reads.
//   * LDS -> lane: the accumulator's key order is groups of four consecutive keys (register r of key block kb: key kb*32 + (r & 3) + 8 (r >> 2) + 4 hi), i.e. eight
//     8-byte reads per lane; s = qk + float(m) * log2 e, one conversion per element (Q carries scale * log2 e, so the scores are in log2 units).
//
// -inf, by construction:
//   * the running max m of a query may still be -inf after a tile (every key so far masked).  The vote of the deferred max, tmax > m + FA_THR, is false for
//     tmax = -inf whatever m is ("no move") and true for a finite tmax over m = -inf.  After the vote, m = -inf implies that every score of this tile is -inf
//     (a finite one in either lane half would have voted), and the exponent is taken against 0 instead: p = exp2(-inf - 0) = 0, never exp2(-inf + inf).
//   * a move out of m = -inf rescales with alpha = 1 (the accumulators are still zero); otherwise alpha = exp2(m - m_new) with both finite.
//   * a row with no live key ends with l = 0 and writes zeros, as the reference implementation's CPU kernel does.
//   * finite large-negative masks (f16 -65504) are ordinary values: they go through the same arithmetic and come out as p = 0 next to any live key.
// No tile skip: a wave-uniform branch around the QK^T, softmax and PV of a tile whose 32 x 64 mask values are all -inf (known when the wave copies the tile to
// LDS) was built and measured (profiles/flash_mask_probe.txt): 4 .. 5 % SLOWER at every probe shape — the test costs every tile a compare per
// element and a vote, and the probe shapes have at most 3 of 68 dead tiles — so it was removed.  A fully masked tile runs through the rules above and adds exact zeros.
// Nothing depends on the grid or on which wave runs first: two runs are bit-equal, and a head computes the same bits whatever else the launch holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "device_utils.h"
#include "kernels.h"

namespace mi355x {

namespace {
constexpr int FM_KT  = 64;  // keys per tile
constexpr int FM_MTS = 68;  // mask tile row stride in halfs
constexpr uint32_t FM_OOR = 0x7fffff00u;  // a buffer offset beyond every descriptor here: the load fetches nothing and returns zeros

struct FMArgs {
    const char *q, *k, *v, *m;
    float* dst;
    int64_t q_nb1, q_nb2, k_nb1, k_nb2, v_nb1, v_nb2, m_nb2, dst_nb_q, dst_nb_h, dst_nb_n;
    int H, Hm;
    int Lq, Lk, Lqm;  // Lqm: rows of one mask plane (>= Lq)
    int grp, units;   // XCD-grouped 1-D grid, as k_flash_attn: heads per unit, (image, query block) units
    int q_vec;        // Q rows 16-byte aligned -> coalesced float4 staging through LDS
    int m_vec;        // Lk % 4 == 0 and the mask 8-byte aligned -> 8-byte mask loads
    float scale_log2e;
};

typedef short fm_short4_t __attribute__((__vector_size__(4 * sizeof(short))));
typedef _Float16 fm_half2_t __attribute__((ext_vector_type(2)));
typedef float fm_float2_t __attribute__((ext_vector_type(2)));
// gfx950 transposing LDS read (see flash_attn.hip): lane i of a 16-lane group addresses 4 consecutive halfs; lane l receives half (l & 3) of the 8 bytes
// addressed by lanes 4 j + ((l & 15) >> 2), j = 0 .. 3
__device__ __forceinline__ half4_t fm_read_tr16(const _Float16* p) {
    const fm_short4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) fm_short4_t*)p);
    return __builtin_bit_cast(half4_t, v);
}
// row stride (halfs) of the row-major V tile: rows 16 dwords apart modulo the 64 banks never collide in the transposing read
constexpr int fm_vtr_stride(int ndv) {
    int dw = ndv * 16;
    if (dw % 64 != 16 && dw % 64 != 48) dw += 16;
    return dw * 2;
}

// Budget (256 threads = 128 queries of one head; compiler's resource report, no scratch):
//   d      K / V tile buffers x 2   mask tile   LDS        workgroups per CU
//   64     43 008 B                 17 408 B    60 416 B   2
//   128    75 776 B                 17 408 B    93 184 B   1   (the unmasked kernel's 75 776 B admit two: the mask tile is what the second one costs)
template <int DKP, int NDV>
__global__ __launch_bounds__(256, DKP <= 64 ? 2 : 1) void k_flash_mask(FMArgs g) {
    static_assert((DKP == 64 && NDV == 2) || (DKP == 128 && NDV == 4), "head dims 64 and 128");
    constexpr int VRS    = fm_vtr_stride(NDV);       // V tile row stride (halfs)
    constexpr int KS     = DKP / 16;                 // MFMA k-steps over the head dim
    constexpr int KROW   = DKP + 8;                  // K tile row stride (halfs)
    constexpr int DCH    = DKP / 8;                  // 16-byte chunks per row
    constexpr int NCH    = FM_KT * DCH / 256;        // prefetched chunks per thread, K and V each (exact)
    constexpr int TILE_H = FM_KT * (KROW + VRS);     // halfs per tile buffer
    constexpr int QWG    = 128;                      // queries per workgroup
    __shared__ __attribute__((aligned(16))) _Float16 smem[2 * TILE_H];
    __shared__ __attribute__((aligned(16))) _Float16 msk[4 * 32 * FM_MTS];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi   = lane >> 5;
    int hn, qb;  // workgroup id -> (head-image, query block), XCD-grouped as in k_flash_attn
    if (g.grp > 0) {
        const int id = blockIdx.x, xcd = id & 7, j = id >> 3;
        const int h = j % g.grp, unit = (j / g.grp) * 8 + xcd;
        if (unit >= g.units) return;
        const int nrb = (g.Lq + QWG - 1) / QWG;
        hn = (unit / nrb) * g.grp + h;
        qb = unit % nrb;
    } else {
        hn = blockIdx.y;
        qb = blockIdx.x;
    }
    const int q0 = qb * QWG + wave * 32;  // first query of this wave
    const int qi = q0 + (lane & 31);

    // ---- Q fragments (B operand of S^T): lane holds Q[qi][ks*16 + hi*8 .. +8] * scale * log2 e as f16
    half8_t qf[KS];
    if (g.q_vec) {  // the workgroup's 128 rows: coalesced float4 loads, handed to the lanes through LDS (the region aliases the K / V tiles, staged afterwards)
        constexpr int QROW = DKP + 4, C4 = DKP / 4;
        static_assert(QWG * QROW <= 2 * TILE_H, "Q staging must fit the K/V tile buffers");
        const char* qblk = g.q + (int64_t)hn * g.q_nb2 + (int64_t)(qb * QWG) * g.q_nb1;
        for (int e = threadIdx.x; e < QWG * C4; e += 256) {
            const int row = e / C4, c4 = e - row * C4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (qb * QWG + row < g.Lq) v = *(const float4*)(qblk + (int64_t)row * g.q_nb1 + c4 * 16);
            half4_t h;
            h[0] = (_Float16)(v.x * g.scale_log2e);
            h[1] = (_Float16)(v.y * g.scale_log2e);
            h[2] = (_Float16)(v.z * g.scale_log2e);
            h[3] = (_Float16)(v.w * g.scale_log2e);
            *(half4_t*)&smem[row * QROW + c4 * 4] = h;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const _Float16* p = &smem[(wave * 32 + (lane & 31)) * QROW + ks * 16 + hi * 8];
            const half4_t a = *(const half4_t*)p, c = *(const half4_t*)(p + 4);
            qf[ks] = (half8_t){a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
        }
        __syncthreads();
    } else {
        const float* qrow = (const float*)(g.q + (int64_t)min(qi, g.Lq - 1) * g.q_nb1 + (int64_t)hn * g.q_nb2);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[ks][j] = (_Float16)(qi < g.Lq ? qrow[ks * 16 + hi * 8 + j] * g.scale_log2e : 0.f);
    }

    float16_t o[NDV];
#pragma unroll
    for (int nb = 0; nb < NDV; ++nb) o[nb] = (float16_t){0};
    float m_run = -INFINITY, l_run = 0.f;

    auto uni_ptr = [](const char* p) {
        const uint64_t u = (uint64_t)(uintptr_t)p;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
        return (const char*)(uintptr_t)(((uint64_t)hi_ << 32) | lo);
    };
    // ---- K / V staging: thread e -> (key = e / DCH, chunk = e % DCH), 16-byte buffer loads through a descriptor of one head's Lk rows (< 2 GiB: the launcher checks),
    // per-lane offsets that never change, the tile offset in an SGPR
    const char* kbase = uni_ptr(g.k + (int64_t)hn * g.k_nb2);
    const char* vbase = uni_ptr(g.v + (int64_t)hn * g.v_nb2);
    const auto rsK = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, (int)((int64_t)g.Lk * g.k_nb1), 0x00020000);
    const auto rsV = __builtin_amdgcn_make_buffer_rsrc((void*)vbase, 0, (int)((int64_t)g.Lk * g.v_nb1), 0x00020000);
    half8_t kreg[NCH], vreg[NCH];
    uint32_t koff[NCH], voff[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int e = threadIdx.x + c * 256, key = e / DCH, ch = e - key * DCH;
        koff[c] = (uint32_t)key * (uint32_t)g.k_nb1 + (uint32_t)ch * 16u;
        voff[c] = (uint32_t)key * (uint32_t)g.v_nb1 + (uint32_t)ch * 16u;
    }
    auto gload = [&](int kt) {
        const int left = g.Lk - kt;
        const int sk = kt * (int)g.k_nb1, sv = kt * (int)g.v_nb1;  // wave-uniform tile offsets
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const bool in = (int)(threadIdx.x + c * 256) / DCH < left;  // keys beyond Lk fetch nothing: their per-lane offset fails the range check by itself
            kreg[c] = __builtin_bit_cast(half8_t, __builtin_amdgcn_raw_buffer_load_b128(rsK, in ? (int)koff[c] : (int)FM_OOR, sk, 0));
            vreg[c] = __builtin_bit_cast(half8_t, __builtin_amdgcn_raw_buffer_load_b128(rsV, in ? (int)voff[c] : (int)FM_OOR, sv, 0));
        }
    };
    auto lstore = [&](int buf, int kt) {
        _Float16* ks = smem + buf * TILE_H;
        _Float16* vt = ks + FM_KT * KROW;
        const int left = g.Lk - kt;
        if (left >= FM_KT) {  // wave-uniform: a full tile is stored as loaded
            asm volatile("" ::: "memory");  // keeps this a branch: if-converted, the two paths merge back into per-element selects
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int e = threadIdx.x + c * 256, key = e / DCH, ch = e - key * DCH;
                *(half8_t*)&ks[key * KROW + ch * 8] = kreg[c];
                *(half8_t*)&vt[key * VRS + ch * 8]  = vreg[c];
            }
            return;
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {  // ragged last tile: keys beyond Lk as zeros (0 * V stays finite; their scores get the mask's -inf)
            const int e = threadIdx.x + c * 256, key = e / DCH, ch = e - key * DCH;
            const half8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
            *(half8_t*)&ks[key * KROW + ch * 8] = key < left ? kreg[c] : z;
            *(half8_t*)&vt[key * VRS + ch * 8]  = key < left ? vreg[c] : z;
        }
    };

    // ---- mask staging: this wave's 32 rows x 64 keys (see the header).  mreg holds a tile in both forms: 8 x 4 halfs.
    const char* mbase = uni_ptr(g.m + (int64_t)(hn % g.Hm) * g.m_nb2);
    const auto rsM    = __builtin_amdgcn_make_buffer_rsrc((void*)mbase, 0, (int)g.m_nb2, 0x00020000);
    _Float16* Mw      = msk + wave * 32 * FM_MTS;
    half4_t mreg[8];
    const _Float16 NINF = (_Float16)(-INFINITY);
    auto mload = [&](int kt) {
        if (g.m_vec) {  // lane -> (row (l >> 4) + 4 it, keys kt + 4 (l & 15) ..)
            const int key = kt + 4 * (lane & 15);
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int row = q0 + 4 * it + (lane >> 4);
                const bool in = key < g.Lk && row < g.Lq;
                const uint32_t off = ((uint32_t)row * (uint32_t)g.Lk + (uint32_t)key) * 2u;
                mreg[it] = __builtin_bit_cast(half4_t, __builtin_amdgcn_raw_buffer_load_b64(rsM, in ? (int)off : (int)FM_OOR, 0, 0));
            }
        } else {  // lane -> key kt + l, row it
            const int key = kt + lane;
#pragma unroll
            for (int it = 0; it < 32; ++it) {
                const int row = q0 + it;
                const bool in = key < g.Lk && row < g.Lq;
                const uint32_t off = ((uint32_t)row * (uint32_t)g.Lk + (uint32_t)key) * 2u;
                mreg[it >> 2][it & 3] = __builtin_bit_cast(_Float16, __builtin_amdgcn_raw_buffer_load_b16(rsM, in ? (int)off : (int)FM_OOR, 0, 0));
            }
        }
    };
    // registers -> LDS; what lies outside the tile's real part becomes -inf
    auto mstore = [&](int kt) {
        if (g.m_vec) {
            const int key = kt + 4 * (lane & 15);
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int row = 4 * it + (lane >> 4);
                const bool in = key < g.Lk && q0 + row < g.Lq;
                *(half4_t*)&Mw[row * FM_MTS + 4 * (lane & 15)] = in ? mreg[it] : (half4_t){NINF, NINF, NINF, NINF};
            }
        } else {
            const int key = kt + lane;
#pragma unroll
            for (int it = 0; it < 32; ++it) {
                const bool in = key < g.Lk && q0 + it < g.Lq;
                Mw[it * FM_MTS + lane] = in ? mreg[it >> 2][it & 3] : NINF;
            }
        }
    };

    mload(0);
    gload(0);
    lstore(0, 0);
    mstore(0);
    if (FM_KT < g.Lk) {
        gload(FM_KT);
        mload(FM_KT);
    }
    __syncthreads();

    // B fragment addressing of the transposing read: 16 keys of k-step t, output columns nb * 32 + (lane & 31), as two 4-key halves (keys t*16 + 4 hi .. and the
    // same 8 further on) — the accumulator's own key order
    const int vtr_lane = (4 * hi + ((lane & 15) >> 2)) * VRS + ((lane >> 4) & 1) * 16 + 4 * (lane & 3);
    int buf = 0;
    for (int kt = 0; kt < g.Lk; kt += FM_KT) {
        // tile kt sits in buffer buf, its mask rows in Mw; the registers hold tile kt + 64: park K / V in the other buffer now, then fetch kt + 128
        if (kt + FM_KT < g.Lk) lstore(buf ^ 1, kt + FM_KT);
        if (kt + 2 * FM_KT < g.Lk) gload(kt + 2 * FM_KT);
        {
            const _Float16* Kc = smem + buf * TILE_H;
            const _Float16* Vc = Kc + FM_KT * KROW;
            auto vread = [&](int t, int nb, half4_t& a, half4_t& c) {
                const _Float16* p = Vc + vtr_lane + t * 16 * VRS + nb * 32;
                a = fm_read_tr16(p);
                c = fm_read_tr16(p + 8 * VRS);
            };
            // ---- S^T = K Q^T (rows = keys, columns = queries), fragment reads ahead of the MFMAs as in k_flash_attn
            float16_t s[2];
            if constexpr (KS == 4) {
                half8_t kf[2][KS];
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) kf[kb][ks] = *(const half8_t*)&Kc[(kb * 32 + (lane & 31)) * KROW + ks * 16 + hi * 8];
                __builtin_amdgcn_sched_barrier(0);
                s[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[0][0], qf[0], (float16_t){0}, 0, 0, 0);
                s[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[1][0], qf[0], (float16_t){0}, 0, 0, 0);
#pragma unroll
                for (int ks = 1; ks < KS; ++ks)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb) s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[kb][ks], qf[ks], s[kb], 0, 0, 0);
            } else {  // d = 128: groups of four fragments, the next group's reads in flight during the current group's MFMAs
                static_assert(KS == 8, "the issue pattern below is written for KS = 8");
                half8_t ka[4], kbq[4];
                auto rdg = [&](half8_t(&dst)[4], int gi) {
                    const int kb = (gi * 4) / KS, ks0 = (gi * 4) % KS;
#pragma unroll
                    for (int j = 0; j < 4; ++j) dst[j] = *(const half8_t*)&Kc[(kb * 32 + (lane & 31)) * KROW + (ks0 + j) * 16 + hi * 8];
                };
                s[0] = (float16_t){0};
                s[1] = (float16_t){0};
                rdg(ka, 0);
#pragma unroll
                for (int gi = 0; gi < 4; gi += 2) {
                    rdg(kbq, gi + 1);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[gi / 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ka[j], qf[j], s[gi / 2], 0, 0, 0);
                    if (gi + 2 < 4) rdg(ka, gi + 2);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[gi / 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kbq[j], qf[4 + j], s[gi / 2], 0, 0, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // ---- this query's mask values in the accumulator's key order, and the first four V fragments: in flight during the softmax
            half4_t mv[2][4];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) mv[kb][gq] = *(const half4_t*)&Mw[(lane & 31) * FM_MTS + kb * 32 + 8 * gq + 4 * hi];
            half4_t vq0[4], vq1[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) vread(i / NDV, i % NDV, vq0[i], vq1[i]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kb][r] = __builtin_fmaf((float)mv[kb][r >> 2][r & 3], 1.44269504088896340736f, s[kb][r]);
            // ---- online softmax of query (lane & 31) with the deferred running max; the -inf rules of the header
            float tmax = s[0][0];
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = __builtin_fmaxf(__builtin_fmaxf(tmax, s[0][r]), s[1][r]);
            if (__any(tmax > m_run + FA_THR)) {  // false for a lane whose 32 scores are all -inf: no move
                tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
                const float m_new = fmaxf(m_run, tmax);  // still -inf for a query with no live key so far
                const float alpha = m_run == -INFINITY ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);  // out of -inf: the accumulators are zero
                m_run             = m_new;
                l_run *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) {  // row (r & 3) + 8 (r >> 2) + 4 hi of the accumulator belongs to the query of that lane
                    const float ar = __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * hi, 64);
#pragma unroll
                    for (int nb = 0; nb < NDV; ++nb) o[nb][r] *= ar;
                }
            }
            const float m_ref = m_run == -INFINITY ? 0.f : m_run;  // m_run = -inf here: every score of this tile is -inf -> p = 0
            float psum        = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[kb][r] = __builtin_amdgcn_exp2f(s[kb][r] - m_ref);
                    psum += s[kb][r];
                }
            l_run += psum;
            half8_t pa[4];  // P in f16, in the accumulator's own key order: the A operand of P V with no data movement
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int kb = t >> 1, rb = (t & 1) * 8;
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    const fm_half2_t h2 = __builtin_convertvector((fm_float2_t){s[kb][rb + j], s[kb][rb + j + 1]}, fm_half2_t);
                    pa[t][j]     = h2[0];
                    pa[t][j + 1] = h2[1];
                }
            }
            // ---- O += P V: 4 k-steps of 16 keys, a ring of four V fragments
            constexpr int NFR = 4 * NDV;
#pragma unroll
            for (int i = 0; i < NFR; ++i) {
                const int t = i / NDV, nb = i % NDV;
                const half4_t v0 = vq0[i & 3], v1 = vq1[i & 3];
                const half8_t vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                o[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pa[t], vf, o[nb], 0, 0, 0);
                if (i + 4 < NFR) vread((i + 4) / NDV, (i + 4) % NDV, vq0[i & 3], vq1[i & 3]);
            }
#pragma unroll
            for (int i = 0; i < NFR; ++i) {  // the fragment's MFMA, then the two reads that refill its ring slot
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (i + 4 < NFR) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
        }
        // the wave is done with its mask rows of tile kt: copy tile kt + 64 over them, fetch kt + 128
        __builtin_amdgcn_wave_barrier();
        if (kt + FM_KT < g.Lk) mstore(kt + FM_KT);
        if (kt + 2 * FM_KT < g.Lk) mload(kt + 2 * FM_KT);
        __syncthreads();  // tile kt + 64 is complete in the other buffer and in Mw; everybody is done reading this one
        buf ^= 1;
    }

    // ---- finalise: divide by the row sum (both lane halves; zero for a row with no live key), write [d] contiguous
    const int hh = g.H > 0 ? hn % g.H : hn, nn = g.H > 0 ? hn / g.H : 0;  // wave-uniform
    char* obase = (char*)g.dst + (int64_t)hh * g.dst_nb_h + (int64_t)nn * g.dst_nb_n;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv   = l_tot > 0.f ? 1.0f / l_tot : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row  = (r & 3) + 8 * (r >> 2) + 4 * hi;
        const float ir = __shfl(inv, row, 64);
        const int q    = q0 + row;
        if (q >= g.Lq) continue;
#pragma unroll
        for (int nb = 0; nb < NDV; ++nb) *(float*)(obase + (int64_t)q * g.dst_nb_q + (nb * 32 + (lane & 31)) * 4) = o[nb][r] * ir;
    }
}
}  // namespace

bool flash_attn_mask_operands_ok(const View4& q, const View4& k, const View4& v, const View4& m) {
    const int64_t D = q.ne[0], Lq = q.ne[1], Lk = k.ne[1];
    auto kv_ok = [&](const View4& t) {  // the FAST form of flash_attn.hip
        return t.type == 1 && t.nb[0] == 2 && t.ne[0] == D && t.ne[1] == Lk && t.ne[2] == q.ne[2] && t.nb[1] >= D * 2 && t.nb[1] % 16 == 0 && t.nb[2] % 16 == 0 &&
               t.ne[1] * t.nb[1] < (int64_t)0x7fffff00;
    };
    const bool q_ok = q.type == 0 && q.nb[0] == 4 && q.nb[1] % 4 == 0 && q.nb[2] % 4 == 0 && q.ne[3] == 1 && Lq >= 1 && Lq < (int64_t)0x7fffff00;
    const bool m_ok = m.type == 1 && m.nb[0] == 2 && m.nb[1] == m.ne[0] * 2 && m.nb[2] == m.nb[1] * m.ne[1] && m.ne[0] == Lk && m.ne[1] >= Lq && m.ne[3] == 1 && m.ne[2] >= 1 &&
                      q.ne[2] % m.ne[2] == 0 && m.nb[2] < (int64_t)0x7fffff00;
    return (D == 64 || D == 128) && Lk >= 1 && q_ok && kv_ok(k) && kv_ok(v) && m_ok;
}

void launch_flash_mask(hipStream_t s, const FlashOut& out, const View4& q, const View4& k, const View4& v, const View4& m, float scale) {
    auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
    if (!flash_attn_mask_operands_ok(q, k, v, m) || !al(k.data, 16) || !al(v.data, 16) || !al(q.data, 4) || !al(m.data, 2) || !out.dst || out.dst16) {
        fprintf(stderr, "mi355x: launch_flash_mask: operands outside the kernel's limits (d %lld, Lq %lld, Lk %lld, mask [%lld, %lld, %lld]; Q f32 and K / V f16 d-contiguous with 16-byte aligned rows, f16 contiguous mask, f32 output)\n",
                (long long)q.ne[0], (long long)q.ne[1], (long long)k.ne[1], (long long)m.ne[0], (long long)m.ne[1], (long long)m.ne[2]);
        abort();
    }
    FMArgs g;
    g.q        = (const char*)q.data;
    g.k        = (const char*)k.data;
    g.v        = (const char*)v.data;
    g.m        = (const char*)m.data;
    g.dst      = out.dst;
    g.H        = out.H;
    g.dst_nb_q = out.nb_q;
    g.dst_nb_h = out.nb_h;
    g.dst_nb_n = out.nb_n;
    g.q_nb1    = q.nb[1];
    g.q_nb2    = q.nb[2];
    g.k_nb1    = k.nb[1];
    g.k_nb2    = k.nb[2];
    g.v_nb1    = v.nb[1];
    g.v_nb2    = v.nb[2];
    g.m_nb2    = m.nb[2];
    g.Hm       = (int)m.ne[2];
    g.Lq       = (int)q.ne[1];
    g.Lk       = (int)k.ne[1];
    g.Lqm      = (int)m.ne[1];
    g.q_vec    = ((((uintptr_t)q.data) | (uintptr_t)q.nb[1] | (uintptr_t)q.nb[2]) & 15) == 0;
    g.m_vec    = g.Lk % 4 == 0 && al(m.data, 8);
    g.scale_log2e = scale * 1.44269504088896340736f;
    g.grp = g.units = 0;
    dim3 grid((unsigned)((g.Lq + 127) / 128), (unsigned)q.ne[2]);
    if (out.H > 0 && q.ne[2] % out.H == 0) {  // XCD-grouped 1-D grid (see k_flash_attn)
        g.grp   = out.H;
        g.units = (int)(q.ne[2] / out.H) * (int)grid.x;
        grid    = dim3((unsigned)(((g.units + 7) / 8) * 8 * g.grp), 1u);
    }
    if (q.ne[0] == 64)
        k_flash_mask<64, 2><<<grid, 256, 0, s>>>(g);
    else
        k_flash_mask<128, 4><<<grid, 256, 0, s>>>(g);
}

}  // namespace mi355x
