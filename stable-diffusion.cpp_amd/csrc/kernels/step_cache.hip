// step_cache.hip — the two device passes of the step caches (EasyCache / UCache, csrc/host/step_cache.hpp) on the device-resident sampler:
//   probe : stats[0] = sum |x * c_in - prev_in|                         (the input change the host state machine decides on)
//   record: diff_j = out_j - in, prev_in = in, prev_out = out_0,
//           stats[1] = sum |out_0 - prev_out(old)|, stats[2] = sum |out_0|   (what after_condition measures, one pass over the step's tensors)
// The sums are DETERMINISTIC: the grid is a function of the element count only, every thread owns a fixed set of elements, a workgroup combines its 256
// accumulators through wave64 shuffles and LDS and stores ONE partial per sum; a second one-workgroup launch adds the partials in a fixed order.  No floating-point
// atomics.  Summation depth of any element: <= SC_ITEMS_MAX additions on a thread's accumulator (+ 2 inside a 16-byte item), 6 across the wave, 2 across the four
// waves, and in the finish pass 4 + 6 + 2 — at most 86 <= 128, so with non-negative terms the relative error is below 128 * 2^-24.
#include "device_utils.h"

namespace mi355x {

constexpr int SC_THREADS    = 256;
constexpr int SC_MAX_BLOCKS = 1024;  // partials per sum: the finish pass reads at most 4 per thread
constexpr int SC_ITEMS      = 4;     // items (16-byte quads or single tail elements) per thread the grid is sized for: the passes sit on the one synchronising
                                     // path of an active step, so the loads are spread over the machine (a 131072-float SD1.5 batch: 32 workgroups, not 4)
constexpr int SC_ITEMS_MAX  = 64;    // ... and the most a thread may get when the grid is capped: larger inputs are refused (launchers return false)

__device__ __forceinline__ float sc_block_sum(float v, float* lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    __syncthreads();
    return r;
}

// x * c_in is ONE rounded f32 multiply (what the step graph's MUL node stores as `noised`), never contracted into the subtraction
__device__ __forceinline__ float sc_absdiff_scaled(float x, float c_in, float p) {
#pragma clang fp contract(off)
    const float m = x * c_in;
    return fabsf(m - p);
}

__global__ __launch_bounds__(SC_THREADS) void k_step_cache_probe(const float* __restrict__ x, float c_in, const float* __restrict__ prev_in, int64_t n, int vec,
                                                                  float* __restrict__ partial) {
    __shared__ float lds[4];
    const int64_t gt = (int64_t)gridDim.x * SC_THREADS, t = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    const int64_t nq = vec ? (n >> 2) : 0;
    float acc        = 0.f;
    for (int64_t q = t; q < nq; q += gt) {
        const float4 a = ((const float4*)x)[q], p = ((const float4*)prev_in)[q];
        acc += (sc_absdiff_scaled(a.x, c_in, p.x) + sc_absdiff_scaled(a.y, c_in, p.y)) + (sc_absdiff_scaled(a.z, c_in, p.z) + sc_absdiff_scaled(a.w, c_in, p.w));
    }
    for (int64_t e = 4 * nq + t; e < n; e += gt) acc += sc_absdiff_scaled(x[e], c_in, prev_in[e]);
    const float s = sc_block_sum(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// in / prev_in / prev_out: [per, nb]; out / diff: [per, k, nb] (the k conditions of an image adjacent, condition 0 first: the step graph's eps layout).
// vec: every base is 16-byte aligned and a quad never straddles an image (per % 4 == 0, or k == 1 where the layouts coincide).
// has_prev_out == 0: prev_out has never been written — it is not read and the first sum is 0.
__global__ __launch_bounds__(SC_THREADS) void k_step_cache_record(const float* __restrict__ in, const float* __restrict__ out, float* __restrict__ prev_in,
                                                                   float* __restrict__ prev_out, float* __restrict__ diff, int64_t per, int k, int64_t nb, int has_prev_out,
                                                                   int vec, float* __restrict__ partial) {
    __shared__ float lds[4];
    const int64_t gt = (int64_t)gridDim.x * SC_THREADS, t = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    const int64_t n  = per * nb;
    const int64_t nq = vec ? (n >> 2) : 0;
    float change = 0.f, norm = 0.f;
    for (int64_t q = t; q < nq; q += gt) {
        const int64_t e = 4 * q;
        int64_t o       = e;
        if (k > 1) {
            const int64_t b = e / per;
            o               = b * k * per + (e - b * per);
        }
        const float4 vi = *(const float4*)(in + e), v0 = *(const float4*)(out + o);
        *(float4*)(diff + o) = make_float4(v0.x - vi.x, v0.y - vi.y, v0.z - vi.z, v0.w - vi.w);
        for (int j = 1; j < k; ++j) {
            const float4 vj                         = *(const float4*)(out + o + (int64_t)j * per);
            *(float4*)(diff + o + (int64_t)j * per) = make_float4(vj.x - vi.x, vj.y - vi.y, vj.z - vi.z, vj.w - vi.w);
        }
        if (has_prev_out) {
            const float4 p = *(const float4*)(prev_out + e);
            change += (fabsf(v0.x - p.x) + fabsf(v0.y - p.y)) + (fabsf(v0.z - p.z) + fabsf(v0.w - p.w));
        }
        norm += (fabsf(v0.x) + fabsf(v0.y)) + (fabsf(v0.z) + fabsf(v0.w));
        *(float4*)(prev_in + e)  = vi;
        *(float4*)(prev_out + e) = v0;
    }
    for (int64_t e = 4 * nq + t; e < n; e += gt) {
        int64_t o = e;
        if (k > 1) {
            const int64_t b = e / per;
            o               = b * k * per + (e - b * per);
        }
        const float vi = in[e], v0 = out[o];
        diff[o] = v0 - vi;
        for (int j = 1; j < k; ++j) diff[o + (int64_t)j * per] = out[o + (int64_t)j * per] - vi;
        if (has_prev_out) change += fabsf(v0 - prev_out[e]);
        norm += fabsf(v0);
        prev_in[e]  = vi;
        prev_out[e] = v0;
    }
    const float s1 = sc_block_sum(change, lds);
    const float s2 = sc_block_sum(norm, lds);
    if (threadIdx.x == 0) {
        partial[blockIdx.x]                 = s1;
        partial[SC_MAX_BLOCKS + blockIdx.x] = s2;
    }
}

// one workgroup: stats[s] = the nblocks partials of sum s, thread t adding partials t, t + 256, t + 512, t + 768 in that order
__global__ __launch_bounds__(SC_THREADS) void k_step_cache_finish(const float* __restrict__ partial, int nblocks, int nsums, float* __restrict__ stats) {
    __shared__ float lds[4];
    for (int s = 0; s < nsums; ++s) {
        float acc = 0.f;
        for (int i = threadIdx.x; i < nblocks; i += SC_THREADS) acc += partial[s * SC_MAX_BLOCKS + i];
        const float r = sc_block_sum(acc, lds);
        if (threadIdx.x == 0) stats[s] = r;
    }
}

size_t step_cache_partial_bytes() { return 2 * SC_MAX_BLOCKS * sizeof(float); }

static inline bool sc_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// blocks for `items` work items, 0 when a thread would get more than SC_ITEMS_MAX of them (the depth bound above would not hold)
static int sc_grid(int64_t items) {
    int64_t blocks = (items + (int64_t)SC_THREADS * SC_ITEMS - 1) / ((int64_t)SC_THREADS * SC_ITEMS);
    if (blocks < 1) blocks = 1;
    if (blocks > SC_MAX_BLOCKS) blocks = SC_MAX_BLOCKS;
    if (items > blocks * SC_THREADS * SC_ITEMS_MAX) return 0;
    return (int)blocks;
}

bool launch_step_cache_probe(hipStream_t s, const float* x, float c_in, const float* prev_in, int64_t n, float* partial, float* stats) {
    if (n < 1) return false;
    const int vec       = sc_aligned16(x) && sc_aligned16(prev_in) ? 1 : 0;
    const int64_t items = vec ? (n >> 2) + (n & 3) : n;
    const int blocks    = sc_grid(items);
    if (!blocks) return false;
    hipLaunchKernelGGL(k_step_cache_probe, dim3(blocks), dim3(SC_THREADS), 0, s, x, c_in, prev_in, n, vec, partial);
    hipLaunchKernelGGL(k_step_cache_finish, dim3(1), dim3(SC_THREADS), 0, s, (const float*)partial, blocks, 1, stats);
    return hipGetLastError() == hipSuccess;
}

bool launch_step_cache_record(hipStream_t s, const float* in, const float* out, float* prev_in, float* prev_out, float* diff, int64_t per, int k, int64_t nb, bool has_prev_out,
                              float* partial, float* stats2) {
    if (per < 1 || nb < 1 || k < 1 || k > 2) return false;
    const int64_t n     = per * nb;
    const int vec       = (sc_aligned16(in) && sc_aligned16(out) && sc_aligned16(prev_in) && sc_aligned16(prev_out) && sc_aligned16(diff) && (per % 4 == 0 || k == 1)) ? 1 : 0;
    const int64_t items = vec ? (n >> 2) + (n & 3) : n;
    const int blocks    = sc_grid(items);
    if (!blocks) return false;
    hipLaunchKernelGGL(k_step_cache_record, dim3(blocks), dim3(SC_THREADS), 0, s, in, out, prev_in, prev_out, diff, per, k, nb, has_prev_out ? 1 : 0, vec, partial);
    hipLaunchKernelGGL(k_step_cache_finish, dim3(1), dim3(SC_THREADS), 0, s, (const float*)partial, blocks, 2, stats2);
    return hipGetLastError() == hipSuccess;
}

}  // namespace mi355x
