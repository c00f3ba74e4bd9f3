// step_cache.hip — the device passes of the step caches (csrc/host/step_cache.hpp) on the device-resident sampler:
//   probe : stats[0] = sum |x * c_in - prev_in|                         (the input change the host state machine decides on; EasyCache / UCache)
//   probe_rel: the same sum and stats[3] = sum |prev_in|                 (the CacheDIT modes' relative residual diff, one pass over the two tensors)
//   record: diff_j = out_j - in, prev_in = in, prev_out = out_0,
//           stats[1] = sum |out_0 - prev_out(old)|, stats[2] = sum |out_0|   (what after_condition measures, one pass over the step's tensors)
// The sums are DETERMINISTIC: the grid is a function of the element count only, every thread owns a fixed set of elements, a workgroup combines its 256
// accumulators through wave64 shuffles and LDS and stores ONE partial per sum; a second one-workgroup launch adds the partials in a fixed order.  No floating-point
// atomics.  Summation depth of any element: <= SC_ITEMS_MAX additions on a thread's accumulator (+ 2 inside a 16-byte item), 6 across the wave, 2 across the four
// waves, and in the finish pass 4 + 6 + 2 — at most 86 <= 128, so with non-negative terms the relative error is below 128 * 2^-24.
//   spectrum_predict: Spectrum's forecast from its ring of denoised tensors — a streaming kernel, no sum across elements (at the end of the file)
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

// probe plus sum |prev_in| from the value already loaded: same grid, same ownership of elements, same depth
__global__ __launch_bounds__(SC_THREADS) void k_step_cache_probe_rel(const float* __restrict__ x, float c_in, const float* __restrict__ prev_in, int64_t n, int vec,
                                                                      float* __restrict__ partial) {
    __shared__ float lds[4];
    const int64_t gt = (int64_t)gridDim.x * SC_THREADS, t = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    const int64_t nq = vec ? (n >> 2) : 0;
    float acc = 0.f, mag = 0.f;
    for (int64_t q = t; q < nq; q += gt) {
        const float4 a = ((const float4*)x)[q], p = ((const float4*)prev_in)[q];
        acc += (sc_absdiff_scaled(a.x, c_in, p.x) + sc_absdiff_scaled(a.y, c_in, p.y)) + (sc_absdiff_scaled(a.z, c_in, p.z) + sc_absdiff_scaled(a.w, c_in, p.w));
        mag += (fabsf(p.x) + fabsf(p.y)) + (fabsf(p.z) + fabsf(p.w));
    }
    for (int64_t e = 4 * nq + t; e < n; e += gt) {
        const float p = prev_in[e];
        acc += sc_absdiff_scaled(x[e], c_in, p);
        mag += fabsf(p);
    }
    const float s1 = sc_block_sum(acc, lds);
    const float s2 = sc_block_sum(mag, lds);
    if (threadIdx.x == 0) {
        partial[blockIdx.x]                 = s1;
        partial[SC_MAX_BLOCKS + blockIdx.x] = s2;
    }
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

// one workgroup: stats[s * stat_stride] = the nblocks partials of sum s, thread t adding partials t, t + 256, t + 512, t + 768 in that order
__global__ __launch_bounds__(SC_THREADS) void k_step_cache_finish(const float* __restrict__ partial, int nblocks, int nsums, float* __restrict__ stats, int stat_stride) {
    __shared__ float lds[4];
    for (int s = 0; s < nsums; ++s) {
        float acc = 0.f;
        for (int i = threadIdx.x; i < nblocks; i += SC_THREADS) acc += partial[s * SC_MAX_BLOCKS + i];
        const float r = sc_block_sum(acc, lds);
        if (threadIdx.x == 0) stats[s * stat_stride] = r;
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
    hipLaunchKernelGGL(k_step_cache_finish, dim3(1), dim3(SC_THREADS), 0, s, (const float*)partial, blocks, 1, stats, 1);
    return hipGetLastError() == hipSuccess;
}

bool launch_step_cache_probe_rel(hipStream_t s, const float* x, float c_in, const float* prev_in, int64_t n, float* partial, float* stats) {
    if (n < 1) return false;
    const int vec       = sc_aligned16(x) && sc_aligned16(prev_in) ? 1 : 0;
    const int64_t items = vec ? (n >> 2) + (n & 3) : n;
    const int blocks    = sc_grid(items);
    if (!blocks) return false;
    hipLaunchKernelGGL(k_step_cache_probe_rel, dim3(blocks), dim3(SC_THREADS), 0, s, x, c_in, prev_in, n, vec, partial);
    hipLaunchKernelGGL(k_step_cache_finish, dim3(1), dim3(SC_THREADS), 0, s, (const float*)partial, blocks, 2, stats, 3);  // stats[0] and stats[3]
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
    hipLaunchKernelGGL(k_step_cache_finish, dim3(1), dim3(SC_THREADS), 0, s, (const float*)partial, blocks, 2, stats2, 1);
    return hipGetLastError() == hipSuccess;
}

// ---- Spectrum's forecast (csrc/host/step_cache.hpp: SpectrumState) ----------------------------------------------------------------------------------------
// out[f] = (1 - w) * (h_last + 0.5 * (h_last - h_prev)) + w * sum_j weights[j] * H_j[f], H_j the j-th oldest slot of the ring.  Every operation is ONE rounded f32
// operation in the order of the host loop's (contraction off), so the device sampler and the host loop forecast the same bits.  Pure streaming: k reads and one
// write per element, 16 bytes per lane where every base and the slot stride allow it; no LDS, nothing shared between elements.  Weights and slot offsets are
// kernel arguments, read with a uniform index.
constexpr int SPECTRUM_MAX_K      = 16;
constexpr int SPECTRUM_MAX_BLOCKS = 2048;  // 256 CUs x 8 workgroups of 256 threads; larger inputs stride over the grid
struct SpectrumArgs {
    float weights[SPECTRUM_MAX_K];
    int64_t offset[SPECTRUM_MAX_K];  // of slot j in floats, oldest first
};

__device__ __forceinline__ float spectrum_mac(float pc, float wj, float h) {
#pragma clang fp contract(off)
    const float m = wj * h;
    return pc + m;
}
__device__ __forceinline__ float spectrum_blend(float pc, float h_last, float h_prev, float w_taylor, float w_cheb) {
#pragma clang fp contract(off)
    const float d  = h_last - h_prev;
    const float e  = 0.5f * d;
    const float pt = h_last + e;
    const float a  = w_taylor * pt;
    const float b  = w_cheb * pc;
    return a + b;
}

__global__ __launch_bounds__(SC_THREADS) void k_spectrum_predict(const float* __restrict__ ring, SpectrumArgs a, int k, float w_taylor, float w_cheb, int64_t n, int vec,
                                                                  float* __restrict__ out) {
    const int64_t gt = (int64_t)gridDim.x * SC_THREADS, t = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    const int64_t nq = vec ? (n >> 2) : 0;
    for (int64_t q = t; q < nq; q += gt) {
        float4 pc   = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 last = pc, prev = pc;
        for (int j = 0; j < k; ++j) {
            const float4 h = ((const float4*)(ring + a.offset[j]))[q];
            const float wj = a.weights[j];
            pc.x = spectrum_mac(pc.x, wj, h.x), pc.y = spectrum_mac(pc.y, wj, h.y), pc.z = spectrum_mac(pc.z, wj, h.z), pc.w = spectrum_mac(pc.w, wj, h.w);
            prev = last, last = h;
        }
        ((float4*)out)[q] = make_float4(spectrum_blend(pc.x, last.x, prev.x, w_taylor, w_cheb), spectrum_blend(pc.y, last.y, prev.y, w_taylor, w_cheb),
                                        spectrum_blend(pc.z, last.z, prev.z, w_taylor, w_cheb), spectrum_blend(pc.w, last.w, prev.w, w_taylor, w_cheb));
    }
    for (int64_t e = 4 * nq + t; e < n; e += gt) {
        float pc = 0.f, last = 0.f, prev = 0.f;
        for (int j = 0; j < k; ++j) {
            const float h = ring[a.offset[j] + e];
            pc            = spectrum_mac(pc, a.weights[j], h);
            prev = last, last = h;
        }
        out[e] = spectrum_blend(pc, last, prev, w_taylor, w_cheb);
    }
}

bool launch_spectrum_predict(hipStream_t s, const float* ring, int64_t slot_stride, const int* order, int k, const float* weights, float w, int64_t n, float* out) {
    if (k < 2 || k > SPECTRUM_MAX_K || n < 1 || slot_stride < n) return false;
    SpectrumArgs a{};
    for (int j = 0; j < k; ++j) {
        if (order[j] < 0 || order[j] >= SPECTRUM_MAX_K) return false;
        a.weights[j] = weights[j];
        a.offset[j]  = (int64_t)order[j] * slot_stride;
    }
    const int vec       = (sc_aligned16(ring) && sc_aligned16(out) && slot_stride % 4 == 0) ? 1 : 0;
    const int64_t items = vec ? (n >> 2) + (n & 3) : n;
    int64_t blocks      = (items + SC_THREADS - 1) / SC_THREADS;
    if (blocks > SPECTRUM_MAX_BLOCKS) blocks = SPECTRUM_MAX_BLOCKS;
    const float w_taylor = 1.0f - w;
    hipLaunchKernelGGL(k_spectrum_predict, dim3((unsigned)blocks), dim3(SC_THREADS), 0, s, ring, a, k, w_taylor, w, n, vec, out);
    return hipGetLastError() == hipSuccess;
}

}  // namespace mi355x
