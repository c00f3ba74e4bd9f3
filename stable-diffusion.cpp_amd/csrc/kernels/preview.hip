// preview.hip — the byte stages of the latent previews (csrc/host/preview.hpp), enqueued on the backend stream between two step graphs:
//   latent_preview: latent [W, H, C, N] f32 planar -> RGB bytes [N][H][W][3], the reference's projection preview (src/runtime/latent-preview.h:401-459):
//                   v = x * in_scale (only when in_scale != 1); r = g = b = 0; for d ascending: r = r + v * proj[d][0], ...; + bias; m * .5f + .5f;
//                   clamp as std::min(1, std::max(0, m)) evaluates it (NaN -> 0, +inf -> 1); byte = (uint8_t)(m * 255), truncation.  No table (C = 3): the three
//                   channels are r, g, b and nothing is added.
//   planar_to_u8  : image [W, H, 3, N] f32 planar -> RGB bytes [N][H][W][3], the decode modes' rule (src/runtime/preprocessing.hpp:27-35): v <= 0 -> 0,
//                   v >= 1 -> 255, else (uint8_t)(v * 255.0f + 0.5f); NaN -> 0.  v = x * in_mul + in_add first when (in_mul, in_add) != (1, 0): the KL-VAE's
//                   (x + 1) / 2 host step as x * 0.5f + 0.5f (the same bits: both halve exactly and round the sum once).
// Every operation is ONE rounded f32 operation (contraction off), so the bytes are those of the host restatement.  Pure streaming: consecutive lanes own consecutive
// pixels (every channel plane is read coalesced); on the vector path a lane owns 4 consecutive pixels of one image — a float4 per plane, its 12 bytes stored as three
// 32-bit words — which needs plane % 4 == 0 and 16-byte aligned bases; otherwise, and for whatever the quads leave, one pixel per lane with byte stores.  The grid
// is a function of the pixel count only.  The projection table arrives as a kernel argument and sits in LDS, filled once per workgroup.
#include "device_utils.h"

namespace mi355x {

constexpr int PV_THREADS    = 256;
constexpr int PV_MAX_BLOCKS = 2048;  // 256 CUs x 8 workgroups; larger inputs stride over the grid
constexpr int PV_MAX_C      = 128;   // table capacity: launchers refuse more channels
struct PreviewTable {
    float proj[PV_MAX_C * 3];  // [c][3]
    float bias[3];
};

__device__ __forceinline__ float pv_mac(float acc, float v, float w) {
#pragma clang fp contract(off)
    const float m = v * w;
    return acc + m;
}
__device__ __forceinline__ float pv_scaled(float x, float s, int scaled) {
#pragma clang fp contract(off)
    return scaled ? x * s : x;
}
// + bias (table only), range change, the reference's clamp, truncation
__device__ __forceinline__ uint32_t pv_proj_byte(float acc, float bias, int has_table) {
#pragma clang fp contract(off)
    float m = has_table ? acc + bias : acc;
    const float h = m * 0.5f;
    m             = h + 0.5f;
    m             = (0.0f < m) ? m : 0.0f;
    m             = (m < 1.0f) ? m : 1.0f;
    const float s = m * 255.0f;
    return (uint32_t)s;
}
__device__ __forceinline__ uint32_t pv_round_byte(float x, float mul, float add, int affine) {
#pragma clang fp contract(off)
    float v = x;
    if (affine) {
        const float h = x * mul;
        v             = h + add;
    }
    if (!(v > 0.0f)) return 0u;
    if (v >= 1.0f) return 255u;
    const float s = v * 255.0f;
    const float r = s + 0.5f;
    return (uint32_t)r;
}
// 12 bytes r0 g0 b0 r1 ... b3 as three little-endian words
__device__ __forceinline__ void pv_store_quad(uint8_t* __restrict__ out, int64_t q, const uint32_t r[4], const uint32_t g[4], const uint32_t b[4]) {
    uint32_t* w = (uint32_t*)out + 3 * q;
    w[0]        = r[0] | (g[0] << 8) | (b[0] << 16) | (r[1] << 24);
    w[1]        = g[1] | (b[1] << 8) | (r[2] << 16) | (g[2] << 24);
    w[2]        = b[2] | (r[3] << 8) | (g[3] << 16) | (b[3] << 24);
}

// x: [plane, C, N]; out: [N * plane][3].  vec: plane % 4 == 0 and both bases aligned (x 16 bytes, out 4): then every pixel is in a quad and the second loop is empty
__global__ __launch_bounds__(PV_THREADS) void k_latent_preview(const float* __restrict__ x, PreviewTable tab, int C, int has_table, float in_scale, int scaled, int64_t plane,
                                                                int64_t N, int vec, uint8_t* __restrict__ out) {
    __shared__ float lds[PV_MAX_C * 3 + 3];
    if (has_table) {
        for (int i = threadIdx.x; i < 3 * C; i += PV_THREADS) lds[i] = tab.proj[i];
        if (threadIdx.x < 3) lds[PV_MAX_C * 3 + threadIdx.x] = tab.bias[threadIdx.x];
    }
    __syncthreads();
    const float b0 = has_table ? lds[PV_MAX_C * 3 + 0] : 0.f, b1 = has_table ? lds[PV_MAX_C * 3 + 1] : 0.f, b2 = has_table ? lds[PV_MAX_C * 3 + 2] : 0.f;
    const int64_t gt = (int64_t)gridDim.x * PV_THREADS, t = (int64_t)blockIdx.x * PV_THREADS + threadIdx.x;
    const int64_t P  = plane * N;
    const int64_t nq = vec ? (P >> 2) : 0, qpp = plane >> 2;  // quads, quads per image
    for (int64_t q = t; q < nq; q += gt) {
        const int64_t im = q / qpp;
        const float* src = x + im * C * plane + 4 * (q - im * qpp);
        float r[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
        if (has_table) {
            for (int d = 0; d < C; ++d) {
                const float4 a   = *(const float4*)(src + (int64_t)d * plane);
                const float v[4] = {pv_scaled(a.x, in_scale, scaled), pv_scaled(a.y, in_scale, scaled), pv_scaled(a.z, in_scale, scaled), pv_scaled(a.w, in_scale, scaled)};
                const float pr = lds[3 * d + 0], pg = lds[3 * d + 1], pb = lds[3 * d + 2];
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = pv_mac(r[j], v[j], pr), g[j] = pv_mac(g[j], v[j], pg), b[j] = pv_mac(b[j], v[j], pb);
            }
        } else {
            const float4 a0 = *(const float4*)src, a1 = *(const float4*)(src + plane), a2 = *(const float4*)(src + 2 * plane);
            r[0] = pv_scaled(a0.x, in_scale, scaled), r[1] = pv_scaled(a0.y, in_scale, scaled), r[2] = pv_scaled(a0.z, in_scale, scaled), r[3] = pv_scaled(a0.w, in_scale, scaled);
            g[0] = pv_scaled(a1.x, in_scale, scaled), g[1] = pv_scaled(a1.y, in_scale, scaled), g[2] = pv_scaled(a1.z, in_scale, scaled), g[3] = pv_scaled(a1.w, in_scale, scaled);
            b[0] = pv_scaled(a2.x, in_scale, scaled), b[1] = pv_scaled(a2.y, in_scale, scaled), b[2] = pv_scaled(a2.z, in_scale, scaled), b[3] = pv_scaled(a2.w, in_scale, scaled);
        }
        uint32_t rb[4], gb[4], bb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rb[j] = pv_proj_byte(r[j], b0, has_table), gb[j] = pv_proj_byte(g[j], b1, has_table), bb[j] = pv_proj_byte(b[j], b2, has_table);
        pv_store_quad(out, q, rb, gb, bb);
    }
    for (int64_t e = 4 * nq + t; e < P; e += gt) {
        const int64_t im = e / plane;
        const float* src = x + im * C * plane + (e - im * plane);
        float r = 0.f, g = 0.f, b = 0.f;
        if (has_table) {
            for (int d = 0; d < C; ++d) {
                const float v = pv_scaled(src[(int64_t)d * plane], in_scale, scaled);
                r = pv_mac(r, v, lds[3 * d + 0]), g = pv_mac(g, v, lds[3 * d + 1]), b = pv_mac(b, v, lds[3 * d + 2]);
            }
        } else {
            r = pv_scaled(src[0], in_scale, scaled), g = pv_scaled(src[plane], in_scale, scaled), b = pv_scaled(src[2 * plane], in_scale, scaled);
        }
        out[3 * e + 0] = (uint8_t)pv_proj_byte(r, b0, has_table);
        out[3 * e + 1] = (uint8_t)pv_proj_byte(g, b1, has_table);
        out[3 * e + 2] = (uint8_t)pv_proj_byte(b, b2, has_table);
    }
}

// x: [plane, 3, N]; out: [N * plane][3]; the same ownership and store shape
__global__ __launch_bounds__(PV_THREADS) void k_planar_to_u8(const float* __restrict__ x, float mul, float add, int affine, int64_t plane, int64_t N, int vec,
                                                              uint8_t* __restrict__ out) {
    const int64_t gt = (int64_t)gridDim.x * PV_THREADS, t = (int64_t)blockIdx.x * PV_THREADS + threadIdx.x;
    const int64_t P  = plane * N;
    const int64_t nq = vec ? (P >> 2) : 0, qpp = plane >> 2;
    for (int64_t q = t; q < nq; q += gt) {
        const int64_t im = q / qpp;
        const float* src = x + im * 3 * plane + 4 * (q - im * qpp);
        const float4 a0 = *(const float4*)src, a1 = *(const float4*)(src + plane), a2 = *(const float4*)(src + 2 * plane);
        const uint32_t rb[4] = {pv_round_byte(a0.x, mul, add, affine), pv_round_byte(a0.y, mul, add, affine), pv_round_byte(a0.z, mul, add, affine), pv_round_byte(a0.w, mul, add, affine)};
        const uint32_t gb[4] = {pv_round_byte(a1.x, mul, add, affine), pv_round_byte(a1.y, mul, add, affine), pv_round_byte(a1.z, mul, add, affine), pv_round_byte(a1.w, mul, add, affine)};
        const uint32_t bb[4] = {pv_round_byte(a2.x, mul, add, affine), pv_round_byte(a2.y, mul, add, affine), pv_round_byte(a2.z, mul, add, affine), pv_round_byte(a2.w, mul, add, affine)};
        pv_store_quad(out, q, rb, gb, bb);
    }
    for (int64_t e = 4 * nq + t; e < P; e += gt) {
        const int64_t im = e / plane;
        const float* src = x + im * 3 * plane + (e - im * plane);
        out[3 * e + 0] = (uint8_t)pv_round_byte(src[0], mul, add, affine);
        out[3 * e + 1] = (uint8_t)pv_round_byte(src[plane], mul, add, affine);
        out[3 * e + 2] = (uint8_t)pv_round_byte(src[2 * plane], mul, add, affine);
    }
}

static inline bool pv_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static int pv_grid(int64_t items) {
    int64_t blocks = (items + PV_THREADS - 1) / PV_THREADS;
    if (blocks < 1) blocks = 1;
    if (blocks > PV_MAX_BLOCKS) blocks = PV_MAX_BLOCKS;
    return (int)blocks;
}

bool launch_latent_preview(hipStream_t s, const float* x, int64_t plane, int c, int64_t n, float in_scale, const float* proj, const float* bias, uint8_t* out) {
    if (!x || !out || plane < 1 || n < 1 || c < 1 || c > PV_MAX_C || (!proj && c != 3)) return false;
    PreviewTable tab{};
    if (proj) {
        for (int i = 0; i < 3 * c; ++i) tab.proj[i] = proj[i];
        for (int i = 0; i < 3; ++i) tab.bias[i] = bias ? bias[i] : 0.0f;
    }
    const int vec       = (plane % 4 == 0 && pv_aligned(x, 16) && pv_aligned(out, 4)) ? 1 : 0;
    const int64_t items = vec ? (plane * n) >> 2 : plane * n;
    hipLaunchKernelGGL(k_latent_preview, dim3(pv_grid(items)), dim3(PV_THREADS), 0, s, x, tab, c, proj ? 1 : 0, in_scale, in_scale != 1.0f ? 1 : 0, plane, n, vec, out);
    return hipGetLastError() == hipSuccess;
}

bool launch_planar_to_u8(hipStream_t s, const float* x, int64_t plane, int64_t n, float in_mul, float in_add, uint8_t* out) {
    if (!x || !out || plane < 1 || n < 1) return false;
    const int vec       = (plane % 4 == 0 && pv_aligned(x, 16) && pv_aligned(out, 4)) ? 1 : 0;
    const int64_t items = vec ? (plane * n) >> 2 : plane * n;
    hipLaunchKernelGGL(k_planar_to_u8, dim3(pv_grid(items)), dim3(PV_THREADS), 0, s, x, in_mul, in_add, (in_mul != 1.0f || in_add != 0.0f) ? 1 : 0, plane, n, vec, out);
    return hipGetLastError() == hipSuccess;
}

}  // namespace mi355x
