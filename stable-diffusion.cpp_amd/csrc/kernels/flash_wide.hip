// flash_wide.hip — softmax(scale * Q K^T) V for head dims beyond k_flash_attn's: 160 < D = DV <= 512, D % 64 == 0 (the KL-VAE mid-block runs ONE head of
// d = 512 over every latent position).  Online softmax, the scores never leave the CU.  Reached through launch_flash_attn (the FLASH_ATTN_EXT node only).
//
// Why a plan of its own: one wave owning 32 queries x 512 output columns would need 256 accumulator registers for O alone, so the 4 waves of a workgroup
// SHARE one block of 32 queries and split the head dim:
//   * S^T = K Q^T is split over d: wave w multiplies the slices [w D/4, (w+1) D/4) of K and Q (D/64 k-steps of v_mfma_f32_32x32x16_f16 on a 32-key tile) and
//     writes its partial 32 x 32 score tile to LDS; after one barrier EVERY wave reads the four partials and adds them in the fixed order ((p0 + p1) + p2) + p3.
//     All four waves then hold bit-identical scores and repeat the softmax (16 v_exp_f32 per lane next to 2 D/64 MFMAs: cheaper than a second exchange of the
//     max, the row sums and P);
//   * O += P V is split over the output columns: wave w keeps the 32-column blocks [w NDV, (w+1) NDV) of O in registers (NDV = ceil(D/128): 64 accumulator
//     registers at d = 512) and reads only those columns of the V tile.
// As in k_flash_attn the product is computed "swapped" (A = K rows, B = Q rows), so a lane holds the scores of ONE query (its MFMA column) for 16 keys and
// its partner lane (l ^ 32) the other 16, and P goes back into the MFMA as the A operand of P V without data movement: the k-slots follow the accumulator's
// key order and V is read with the same permutation (ds_read_b64_tr_b16 on the row-major tile).
// Tiles: 32 keys x D of K and of V (f16, 16-byte buffer loads, register-prefetched one tile ahead, two LDS buffers), two barriers per tile (the exchange;
// the end of the tile).  32-key tiles are what fits: at d = 512 two buffers of K + V are 133 KB, the partials 16 KB (64-key tiles: 266 KB).
// Numerics: Q (pre-multiplied by scale * log2 e), K, P and V enter the MFMA as f16; scores, max, sums and O are f32; the running max is deferred by FA_THR
// exactly as in k_flash_attn (P <= 2^8), the first tile takes alpha = 1, keys beyond Lk are masked with -inf (their K / V rows are read as zeros by the
// buffer range check), O is normalised once at the end.  Nothing depends on the grid or on which wave runs first: two runs are bit-equal, and a head
// computes the same bits whatever else the launch holds.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "device_utils.h"
#include "kernels.h"

namespace mi355x {

namespace {
constexpr int FW_KT = 32;  // keys per tile
constexpr int FW_QB = 32;  // queries per workgroup

struct FWArgs {
    const char *q, *k, *v;
    float* dst;
    _Float16* dst16;
    int64_t q_nb1, q_nb2, k_nb1, k_nb2, v_nb1, v_nb2, dst_nb_q, dst_nb_h, dst_nb_n, ld16;
    int H;
    int Lq, Lk;
    int grp, units;  // XCD-grouped 1-D grid, as k_flash_attn: heads per unit, (image, query block) units
    int q_vec;       // Q rows 16-byte aligned -> float4 loads
    float scale_log2e;
};

typedef short fw_short4_t __attribute__((__vector_size__(4 * sizeof(short))));
// gfx950 transposing LDS read (see flash_attn.hip): lane i of a 16-lane group addresses 4 consecutive halfs; lane l receives half (l & 3) of the 8 bytes
// addressed by lanes 4 j + ((l & 15) >> 2), j = 0 .. 3
__device__ __forceinline__ half4_t fw_read_tr16(const _Float16* p) {
    const fw_short4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) fw_short4_t*)p);
    return __builtin_bit_cast(half4_t, v);
}
// row stride (halfs) of the row-major V tile of nb 32-column blocks: a 32-lane half of the transposing read covers 4 keys x 32 columns (64 bytes per key), so
// rows 16 dwords apart modulo the 64 banks never collide
constexpr int fw_vtr_stride(int nb) {
    int dw = nb * 16;
    if (dw % 64 != 16 && dw % 64 != 48) dw += 16;
    return dw * 2;
}

// Budget per instantiation (one workgroup = 256 threads = 32 queries of one head):
//   D      K row / V row (halfs)   tile buffers x 2   partials   LDS      O / Q / prefetch registers per lane   VGPRs + AGPRs (compiler, no scratch)
//   192    200 / 224               54 272 B           16 384 B   69 KB    32 / 12 / 24                          191 + 0
//   256    264 / 288               70 656 B           16 384 B   85 KB    32 / 16 / 32                          174 + 48
//   320    328 / 352               87 040 B           16 384 B   101 KB   48 / 20 / 40                          250 + 64
//   384    392 / 416               103 424 B          16 384 B   117 KB   48 / 24 / 48                          235 + 64
//   448    456 / 480               119 808 B          16 384 B   133 KB   64 / 28 / 56                          256 + 101
//   512    520 / 544               136 192 B          16 384 B   149 KB   64 / 32 / 64                          256 + 93
// d = 192 leaves room for two workgroups per CU (2 waves per SIMD), everything above runs one (1 wave per SIMD: the LDS decides, not the registers).
template <int D>
__global__ __launch_bounds__(256, D <= 192 ? 2 : 1) void k_flash_wide(FWArgs g) {
    static_assert(D % 64 == 0 && D > 160 && D <= 512, "head dims 192 .. 512 in steps of 64");
    constexpr int DW     = D / 4;                 // d slice of one wave in K Q^T
    constexpr int KS     = DW / 16;               // its MFMA k-steps
    constexpr int NB     = D / 32;                // 32-column blocks of O
    constexpr int NDV    = (NB + 3) / 4;          // ... per wave (the last waves own fewer where NB % 4 != 0)
    constexpr int KROW   = D + 8;                 // K tile row stride (halfs): rows 4 dwords apart modulo the banks
    constexpr int VRS    = fw_vtr_stride(NB);     // V tile row stride (halfs)
    constexpr int DCH    = D / 8;                 // 16-byte chunks per row
    constexpr int NCH    = FW_KT * DCH / 256;     // chunks per thread and tile, K and V each (exact: D % 64 == 0)
    constexpr int TILE_H = FW_KT * (KROW + VRS);  // halfs per tile buffer
    static_assert(NCH * 256 == FW_KT * DCH, "every thread stages the same number of chunks");
    __shared__ __attribute__((aligned(16))) _Float16 smem[2 * TILE_H];
    __shared__ __attribute__((aligned(16))) float4 part[4 * 4 * 64];  // [wave][register quad][lane]: the partial score tiles

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi   = lane >> 5;
    // workgroup id -> (head-image hn, query block), XCD-grouped as in k_flash_attn
    int hn, qb;
    if (g.grp > 0) {
        const int id = blockIdx.x, xcd = id & 7, j = id >> 3;
        const int h = j % g.grp, unit = (j / g.grp) * 8 + xcd;
        if (unit >= g.units) return;
        const int nrb = (g.Lq + FW_QB - 1) / FW_QB;
        hn = (unit / nrb) * g.grp + h;
        qb = unit % nrb;
    } else {
        hn = blockIdx.y;
        qb = blockIdx.x;
    }
    const int q0 = qb * FW_QB;

    // ---- Q fragments (B operand of S^T): lane holds Q[q0 + (lane & 31)][wave * DW + ks * 16 + hi * 8 .. + 8] * scale * log2 e as f16.  Read once per workgroup,
    // straight from global memory: 2 KB per row next to the Lk x 2 KB that every row's keys and values stream
    half8_t qf[KS];
    {
        const float* qp = (const float*)(g.q + (int64_t)hn * g.q_nb2 + (int64_t)min(q0 + (lane & 31), g.Lq - 1) * g.q_nb1) + wave * DW + hi * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            float x[8];
            if (g.q_vec) {
                const float4 a = *(const float4*)(qp + ks * 16), b = *(const float4*)(qp + ks * 16 + 4);
                x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w, x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = qp[ks * 16 + j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[ks][j] = (_Float16)(x[j] * g.scale_log2e);  // scores come out of the MFMA in log2 units
        }
    }

    float16_t o[NDV];
#pragma unroll
    for (int j = 0; j < NDV; ++j) o[j] = (float16_t){0};
    float m_run = -INFINITY, l_run = 0.f;

    // ---- staging: thread e -> (key = e / DCH, chunk = e % DCH).  Buffer loads through a wave-uniform descriptor of one head's Lk rows: keys beyond Lk read as zeros,
    // so a ragged last tile needs no select (a zero V row keeps 0 * V finite, the scores of those keys are masked below)
    auto uni_ptr = [](const char* p) {
        const uint64_t u = (uint64_t)(uintptr_t)p;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
        return (const char*)(uintptr_t)(((uint64_t)hi_ << 32) | lo);
    };
    const char* kbase = uni_ptr(g.k + (int64_t)hn * g.k_nb2);
    const char* vbase = uni_ptr(g.v + (int64_t)hn * g.v_nb2);
    const auto rsK = __builtin_amdgcn_make_buffer_rsrc((void*)kbase, 0, (int)((int64_t)g.Lk * g.k_nb1), 0x00020000);  // (< 2 GiB: flash_attn_wide_operands_ok)
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
        const int sk = kt * (int)g.k_nb1, sv = kt * (int)g.v_nb1;  // wave-uniform tile offsets
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            kreg[c] = __builtin_bit_cast(half8_t, __builtin_amdgcn_raw_buffer_load_b128(rsK, (int)koff[c], sk, 0));
            vreg[c] = __builtin_bit_cast(half8_t, __builtin_amdgcn_raw_buffer_load_b128(rsV, (int)voff[c], sv, 0));
        }
    };
    auto lstore = [&](int buf, int kt) {
        _Float16* ks = smem + buf * TILE_H;
        _Float16* vt = ks + FW_KT * KROW;
        const int left = g.Lk - kt;  // keys of a ragged last tile beyond Lk are stored as zeros whatever the load returned (as k_flash_attn's lstore does next to the range check)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int e = threadIdx.x + c * 256, key = e / DCH, ch = e - key * DCH;
            const half8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
            *(half8_t*)&ks[key * KROW + ch * 8] = key < left ? kreg[c] : z;
            *(half8_t*)&vt[key * VRS + ch * 8]  = key < left ? vreg[c] : z;
        }
    };
    gload(0);
    lstore(0, 0);
    if (FW_KT < g.Lk) gload(FW_KT);
    __syncthreads();

    // B fragment addressing of the transposing read: 16 keys of k-step t, output columns nb * 32 + (lane & 31), as two 4-key halves (keys t*16 + 4 hi .. and the
    // same 8 further on) — the accumulator's own key order
    const int vtr_lane = (4 * hi + ((lane & 15) >> 2)) * VRS + ((lane >> 4) & 1) * 16 + 4 * (lane & 3);
    int buf = 0;
    auto tile = [&](const int kt, auto tail_tag) {
        constexpr bool TAIL = decltype(tail_tag)::value;
        // tile kt sits in buffer buf; the registers hold tile kt + 32: park it in the other buffer (free since the barrier that ended the previous tile), fetch kt + 64
        if (kt + FW_KT < g.Lk) lstore(buf ^ 1, kt + FW_KT);
        if (kt + 2 * FW_KT < g.Lk) gload(kt + 2 * FW_KT);
        const _Float16* Kc = smem + buf * TILE_H;
        const _Float16* Vc = Kc + FW_KT * KROW;

        // ---- this wave's share of S^T = K Q^T: keys x queries over its d slice; all K fragments requested before the first MFMA
        half8_t kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = *(const half8_t*)&Kc[(lane & 31) * KROW + wave * DW + ks * 16 + hi * 8];
        float16_t s = (float16_t){0};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qf[ks], s, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) part[(wave * 4 + i) * 64 + lane] = make_float4(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]);
        __syncthreads();
        // ---- every wave: the four partials in one fixed order -> the same bits in all of them
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 p0 = part[(0 * 4 + i) * 64 + lane], p1 = part[(1 * 4 + i) * 64 + lane], p2 = part[(2 * 4 + i) * 64 + lane], p3 = part[(3 * 4 + i) * 64 + lane];
            s[4 * i]     = ((p0.x + p1.x) + p2.x) + p3.x;
            s[4 * i + 1] = ((p0.y + p1.y) + p2.y) + p3.y;
            s[4 * i + 2] = ((p0.z + p1.z) + p2.z) + p3.z;
            s[4 * i + 3] = ((p0.w + p1.w) + p2.w) + p3.w;
        }
        // this wave's V fragments: in flight during the softmax
        half4_t v0[2][NDV], v1[2][NDV];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < NDV; ++j) {
                const int nb = wave * NDV + j;
                if (NB % 4 == 0 || nb < NB) {  // wave-uniform
                    const _Float16* p = Vc + vtr_lane + t * 16 * VRS + nb * 32;
                    v0[t][j] = fw_read_tr16(p);
                    v1[t][j] = fw_read_tr16(p + 8 * VRS);
                } else {
                    v0[t][j] = v1[t][j] = (half4_t){0, 0, 0, 0};
                }
            }
        if (TAIL) {  // register r of this lane: key (r & 3) + 8 (r >> 2) + 4 hi of the tile
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt + (r & 3) + 8 * (r >> 2) + 4 * hi >= g.Lk) s[r] = -INFINITY;
        }
        // ---- online softmax of query (lane & 31), the running max deferred as in k_flash_attn: it moves only when some row's tile max exceeds it by more than FA_THR
        float tmax = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = __builtin_fmaxf(tmax, s[r]);
        if (kt == 0 || __any(tmax > m_run + FA_THR)) {
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(m_run, tmax);
            // first tile: the accumulators are zero and m_run is -inf; alpha = 1 keeps 0 * 2^(-inf - m) out of the arithmetic whatever the first max is
            const float alpha = kt == 0 ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);
            m_run             = m_new;
            l_run *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) {  // row (r & 3) + 8 (r >> 2) + 4 hi of the accumulator belongs to the query of that lane
                const float ar = __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * hi, 64);
#pragma unroll
                for (int j = 0; j < NDV; ++j) o[j][r] *= ar;
            }
        }
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(s[r] - m_run);
            psum += s[r];
        }
        l_run += psum;
        half8_t pa[2];  // P as f16 in the accumulator's key order: the A operand of P V
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j) pa[t][j] = (_Float16)s[8 * t + j];
        // ---- O += P V on this wave's columns
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < NDV; ++j) {
                const half4_t a = v0[t][j], c = v1[t][j];
                const half8_t vf = {a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
                if (NB % 4 == 0 || wave * NDV + j < NB) o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pa[t], vf, o[j], 0, 0, 0);
            }
        __syncthreads();  // tile kt + 32 is complete in the other buffer; everybody is done with this one and with the partials
        buf ^= 1;
    };
    {
        int kt = 0;
        for (; kt + FW_KT <= g.Lk; kt += FW_KT) tile(kt, std::false_type{});
        if (kt < g.Lk) tile(kt, std::true_type{});
    }

    // ---- finalise: divide by the row sum (both lane halves), write this wave's columns d-contiguous
    const int hh = g.H > 0 ? hn % g.H : hn, nn = g.H > 0 ? hn / g.H : 0;  // wave-uniform
    char* obase       = g.dst ? (char*)g.dst + (int64_t)hh * g.dst_nb_h + (int64_t)nn * g.dst_nb_n : nullptr;
    _Float16* obase16 = g.dst16 ? g.dst16 + (int64_t)nn * g.Lq * g.ld16 + (int64_t)hh * D : nullptr;
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv   = l_tot > 0.f ? 1.0f / l_tot : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row  = (r & 3) + 8 * (r >> 2) + 4 * hi;
        const float ir = __shfl(inv, row, 64);
        const int q    = q0 + row;
        if (q >= g.Lq) continue;
#pragma unroll
        for (int j = 0; j < NDV; ++j) {
            const int nb = wave * NDV + j;
            if (NB % 4 != 0 && nb >= NB) continue;
            const int d     = nb * 32 + (lane & 31);
            const float val = o[j][r] * ir;
            if (obase) *(float*)(obase + (int64_t)q * g.dst_nb_q + d * 4) = val;
            if (obase16) obase16[(int64_t)q * g.ld16 + d] = (_Float16)val;
        }
    }
}
}  // namespace

bool flash_attn_wide_supported(int64_t D, int64_t DV) { return D == DV && D > 160 && D <= 512 && D % 64 == 0; }

bool flash_attn_wide_operands_ok(const View4& q, const View4& k, const View4& v) {
    auto kv_ok = [&](const View4& t) {
        return t.type == 1 && t.nb[0] == 2 && t.ne[0] == q.ne[0] && t.ne[1] == k.ne[1] && t.ne[2] == q.ne[2] && t.nb[1] >= t.ne[0] * 2 && t.nb[1] % 16 == 0 && t.nb[2] % 16 == 0 &&
               t.ne[1] * t.nb[1] < (int64_t)0x7fffffff;
    };
    return q.type == 0 && q.nb[0] == 4 && q.nb[1] % 4 == 0 && q.nb[2] % 4 == 0 && q.ne[1] >= 1 && k.ne[1] >= 1 && q.ne[1] < (int64_t)0x7fffffff && kv_ok(k) && kv_ok(v);
}

void launch_flash_wide(hipStream_t s, const FlashOut& out, const View4& q, const View4& k, const View4& v, float scale) {
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    if (!flash_attn_wide_supported(q.ne[0], v.ne[0]) || !flash_attn_wide_operands_ok(q, k, v) || !al16(k.data) || !al16(v.data) || (!out.dst && !out.dst16)) {
        fprintf(stderr, "mi355x: launch_flash_wide: operands outside the kernel's limits (d %lld, Lq %lld, Lk %lld; Q f32 d-contiguous, K / V f16 d-contiguous with 16-byte aligned rows)\n",
                (long long)q.ne[0], (long long)q.ne[1], (long long)k.ne[1]);
        abort();
    }
    FWArgs g;
    g.q        = (const char*)q.data;
    g.k        = (const char*)k.data;
    g.v        = (const char*)v.data;
    g.dst      = out.dst;
    g.dst16    = (_Float16*)out.dst16;
    g.ld16     = out.ld16;
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
    g.Lq       = (int)q.ne[1];
    g.Lk       = (int)k.ne[1];
    g.q_vec    = ((((uintptr_t)q.data) | (uintptr_t)q.nb[1] | (uintptr_t)q.nb[2]) & 15) == 0;
    g.scale_log2e = scale * 1.44269504088896340736f;
    g.grp = g.units = 0;
    dim3 grid((unsigned)((g.Lq + FW_QB - 1) / FW_QB), (unsigned)q.ne[2]);
    if (out.H > 0 && q.ne[2] % out.H == 0) {  // XCD-grouped 1-D grid (see k_flash_attn)
        g.grp   = out.H;
        g.units = (int)(q.ne[2] / out.H) * (int)grid.x;
        grid    = dim3((unsigned)(((g.units + 7) / 8) * 8 * g.grp), 1u);
    }
    switch ((int)q.ne[0]) {
        case 192: k_flash_wide<192><<<grid, 256, 0, s>>>(g); break;
        case 256: k_flash_wide<256><<<grid, 256, 0, s>>>(g); break;
        case 320: k_flash_wide<320><<<grid, 256, 0, s>>>(g); break;
        case 384: k_flash_wide<384><<<grid, 256, 0, s>>>(g); break;
        case 448: k_flash_wide<448><<<grid, 256, 0, s>>>(g); break;
        default: k_flash_wide<512><<<grid, 256, 0, s>>>(g); break;
    }
}

}  // namespace mi355x
