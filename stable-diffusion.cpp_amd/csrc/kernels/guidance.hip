// guidance.hip — the two glue stages the device-resident sampler puts around an inpaint / pix2pix UNet (gfx950), one launch each (planner: plan_model_input,
// plan_guidance3):
//   k_model_input  x * c_in tiled over the K branches of every image, with the branch's constant concat latent appended along the channels
//                  (MUL -> RESHAPE -> REPEAT -> RESHAPE, [REPEAT,] CONCAT dim 2 as plain nodes: 4 launches and three intermediates)
//   k_guidance3    the three-conditioning CFG combine iu + img * (u - iu) + txt * (c - u) (SUB, MUL, ADD, SUB, MUL, ADD as plain nodes: 6 launches)
// Pure streaming kernels judged against the HBM roofline: no LDS, one thread per 16 bytes where the layout allows, grid capped and grid-strided like the other
// elementwise launchers.  Every per-step scalar is READ FROM DEVICE MEMORY: the step graph is replayed as a captured hipGraph, so a launch argument would be frozen.
#include "kernels.h"
#include "ktime.h"

#include <atomic>

namespace mi355x {

static std::atomic<int64_t> g_model_input_launches[2];  // [0] float4 route, [1] scalar route: counted per launch call where the launcher chooses
int64_t model_input_route_launches(int route) { return route >= 0 && route < 2 ? g_model_input_launches[route].load(std::memory_order_relaxed) : 0; }

static inline int stream_grid(int64_t n, int block) {
    const int64_t g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > 256 * 16 ? 256 * 16 : g));
}

// out [plane, C + cc, K * nb]: plane p < C of model image m = b * K + j is x[b] plane p times *scale (scale NULL: copied), plane p >= C is plane p - C of concat
// row m % rows (rows = K: one row per branch, shared by the images; rows = K * nb: one per model image).  V floats per thread; planeV = plane / V.
template <int V>
__global__ void k_model_input(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ cat, int64_t planeV, int C, int cc,
                              int K, int64_t rows, int64_t total) {
    const float s        = scale ? *scale : 1.0f;
    const int CT         = C + cc;
    const int64_t plane  = planeV * V;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pv = i % planeV;
        const int64_t q  = i / planeV;
        const int p      = (int)(q % CT);
        const int64_t m  = q / CT;
        float* dst       = out + (m * CT + p) * plane + pv * V;
        if (p < C) {
            const float* src = x + ((m / K) * C + p) * plane + pv * V;
            if constexpr (V == 4) {
                float4 v = *(const float4*)src;
                if (scale) v.x *= s, v.y *= s, v.z *= s, v.w *= s;
                *(float4*)dst = v;
            } else {
                *dst = scale ? *src * s : *src;
            }
        } else {
            const float* src = cat + ((m % rows) * cc + (p - C)) * plane + pv * V;
            if constexpr (V == 4)
                *(float4*)dst = *(const float4*)src;
            else
                *dst = *src;
        }
    }
}

void launch_model_input(hipStream_t s, float* out, const float* x, const float* scale, const float* cat, int64_t plane, int C, int cc, int K, int64_t nb, int64_t rows) {
    const int64_t images = (int64_t)K * nb;
    if (plane <= 0 || C < 1 || cc < 1 || K < 1 || nb < 1 || rows < 1) return;
    // float4: every plane starts 16-byte aligned when the bases are and the plane is a multiple of 4 floats
    const bool v4 = plane % 4 == 0 && ((((uintptr_t)out | (uintptr_t)x | (uintptr_t)cat) & 15) == 0);
    const int V   = v4 ? 4 : 1;
    const int64_t total = plane / V * (C + cc) * images;
    KScope ks_(s, KF_CONCAT, 0.0, (double)plane * (C + cc) * images * 8.0);  // every output cell is one read and one write
    g_model_input_launches[v4 ? 0 : 1].fetch_add(1, std::memory_order_relaxed);
    if (v4)
        k_model_input<4><<<stream_grid(total, 256), 256, 0, s>>>(out, x, scale, cat, plane / 4, C, cc, K, rows, total);
    else
        k_model_input<1><<<stream_grid(total, 256), 256, 0, s>>>(out, x, scale, cat, plane, C, cc, K, rows, total);
}

// out [per, nb] from e3 [per, 3, nb] (cond, uncond, img_uncond adjacent per image); *txt / *img: the two scales in the step's scalar tensor
template <int V>
__global__ void k_guidance3(float* __restrict__ out, const float* __restrict__ e3, const float* __restrict__ txt, const float* __restrict__ img, int64_t perV, int64_t total) {
    // six separately rounded operations, left to right, like the nodes this launch replaces and like sd::Tensor's operators on the host: hipcc contracts a + b * c
    // into one fused operation by default and this toolchain's __fmul_rn / __fadd_rn are plain operators compiled under that default — the pragma keeps them apart
#pragma clang fp contract(off)
    const float st = *txt, si = *img;
    const int64_t per = perV * V;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / perV, f = (i % perV) * V;
        const float* base = e3 + b * 3 * per + f;
        float c[V], u[V], iu[V], r[V];
        if constexpr (V == 4) {
            const float4 a = *(const float4*)base, d = *(const float4*)(base + per), e = *(const float4*)(base + 2 * per);
            c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = a.w;
            u[0] = d.x, u[1] = d.y, u[2] = d.z, u[3] = d.w;
            iu[0] = e.x, iu[1] = e.y, iu[2] = e.z, iu[3] = e.w;
        } else {
            c[0] = base[0], u[0] = base[per], iu[0] = base[2 * per];
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float d1 = u[k] - iu[k];
            const float s1 = d1 * si;
            const float a1 = iu[k] + s1;
            const float d2 = c[k] - u[k];
            const float s2 = d2 * st;
            r[k]           = a1 + s2;
        }
        float* dst = out + b * per + f;
        if constexpr (V == 4)
            *(float4*)dst = make_float4(r[0], r[1], r[2], r[3]);
        else
            *dst = r[0];
    }
}

void launch_guidance3(hipStream_t s, float* out, const float* e3, const float* txt, const float* img, int64_t per, int64_t nb) {
    if (per <= 0 || nb <= 0) return;
    const bool v4 = per % 4 == 0 && ((((uintptr_t)out | (uintptr_t)e3) & 15) == 0);
    const int V   = v4 ? 4 : 1;
    const int64_t total = per / V * nb;
    KScope ks_(s, KF_BINARY, 0.0, (double)per * nb * 16.0);  // three reads and one write per cell
    if (v4)
        k_guidance3<4><<<stream_grid(total, 256), 256, 0, s>>>(out, e3, txt, img, per / 4, total);
    else
        k_guidance3<1><<<stream_grid(total, 256), 256, 0, s>>>(out, e3, txt, img, per, total);
}

}  // namespace mi355x
