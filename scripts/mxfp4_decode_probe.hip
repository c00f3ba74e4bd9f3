// mxfp4_decode_probe.hip — the measurement behind the MXFP4 decode route (kernels/mxfp4_decode.h).
//   1. Both routes on all 256 exponents x 16 codes against w16 = f16(kvalues[q] * 2^(e - 128)) formed on the host: every pair that differs is printed with what
//      the route returned (bits), grouped by exponent.  The hardware route is run with two scale encodings for e = 0 (2^-127 is an f32 subnormal).
//   2. Decode rate of each route: 256 lanes x many blocks from a cache-resident buffer, 16 weights per lane and block, the results folded into a checksum.
//      Median of 7 launches with min .. max after 2 warm-up launches.
// Build and run:  hipcc -O3 --offload-arch=gfx950 -I stable-diffusion.cpp_amd/csrc/kernels scripts/mxfp4_decode_probe.hip -o mxfp4_decode_probe && ./mxfp4_decode_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include "mxfp4_decode.h"

using namespace mi355x;

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

// out[route][e][q]: route 0 integer, 1 hardware (e = 0 as the subnormal 2^-127), 2 hardware (scale bits e << 23 throughout)
__global__ void k_pairs(uint16_t* out) {
    const uint32_t e = blockIdx.x, q = threadIdx.x;  // 256 x 16
    mx4_half2_t a, b;
    mx4_w4(q, mx4_prep(e), a, b);
    out[e * 16 + q] = __builtin_bit_cast(uint16_t, a[0]);
    mx4_hw4(q, mx4_hw_scale(e), a, b);
    out[4096 + e * 16 + q] = __builtin_bit_cast(uint16_t, a[0]);
    mx4_hw4(q, __builtin_bit_cast(float, e << 23), a, b);
    out[8192 + e * 16 + q] = __builtin_bit_cast(uint16_t, a[0]);
}

template <int HW>
__global__ __launch_bounds__(256) void k_rate(const uint32_t* __restrict__ blocks, int nblk, int iters, uint32_t* sink) {
    uint32_t acc = 0;
    for (int it = 0; it < iters; ++it)
        for (int b = threadIdx.x; b < nblk; b += 256) {  // 3 dwords per block: e, 8 code bytes
            const uint32_t e = blocks[3 * b] & 0xFFu, qa = blocks[3 * b + 1] + it, qb = blocks[3 * b + 2];
            const uint32_t q[4] = {qa & 0x0F0F0F0Fu, qb & 0x0F0F0F0Fu, (qa >> 4) & 0x0F0F0F0Fu, (qb >> 4) & 0x0F0F0F0Fu};
            const MX4Scale m = mx4_prep(e);
            const float sc   = mx4_hw_scale(e);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mx4_half2_t h0, h1;
                if (HW) mx4_hw4(q[j], sc, h0, h1);
                else mx4_w4(q[j], m, h0, h1);
                acc += __builtin_bit_cast(uint32_t, h0) ^ (__builtin_bit_cast(uint32_t, h1) * 3u);
            }
        }
    if (acc == 0x12345u) sink[blockIdx.x] = acc;  // keeps the loop alive
}

static uint16_t ref_bits(int e, int q) {
    static const int kv[16] = {0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12};
    const uint32_t db = e < 2 ? 0x00200000u << e : (uint32_t)(e - 1) << 23;
    float d;
    memcpy(&d, &db, 4);
    const _Float16 h = (_Float16)((float)kv[q] * d);  // round to nearest even
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

int main() {
    uint16_t* dout;
    CHECK(hipMalloc(&dout, 3 * 4096 * 2));
    k_pairs<<<256, 16>>>(dout);
    std::vector<uint16_t> out(3 * 4096);
    CHECK(hipMemcpy(out.data(), dout, out.size() * 2, hipMemcpyDeviceToHost));
    const char* names[3] = {"integer route", "hardware route, e = 0 as subnormal 2^-127", "hardware route, scale bits e << 23"};
    for (int r = 0; r < 3; ++r) {
        int bad_finite = 0, bad_other = 0;
        printf("== %s\n", names[r]);
        for (int e = 0; e < 256; ++e) {
            char line[1024];
            int len = 0;
            for (int q = 0; q < 16; ++q) {
                const uint16_t want = ref_bits(e, q), got = out[r * 4096 + e * 16 + q];
                const bool zero = !(want & 0x7FFF) && !(got & 0x7FFF);  // +0 and -0 are the same weight
                if (want == got || zero) continue;
                const bool finite = (want & 0x7C00) != 0x7C00;
                (finite ? bad_finite : bad_other)++;
                len += snprintf(line + len, sizeof(line) - len, " q%d:%04x(want %04x%s)", q, got, want, finite ? "" : ",nonfinite");
            }
            if (len) printf("  e=%3d (2^%d):%s\n", e, e - 128, line);
        }
        printf("  -> %d pairs differ where f16(y) is finite, %d where it is not\n", bad_finite, bad_other);
    }
    // ---- rate
    const int nblk = 8192, iters = 2000, grid = 1024;  // 96 KiB of blocks (cache-resident), 16 weights per lane and block
    std::vector<uint32_t> hb(3 * nblk);
    uint32_t s = 12345u;
    for (auto& v : hb) v = (s = s * 1664525u + 1013904223u);
    for (int b = 0; b < nblk; ++b) hb[3 * b] = 100 + hb[3 * b] % 40;  // exponents around the f16 range
    uint32_t *dblk, *dsink;
    CHECK(hipMalloc(&dblk, hb.size() * 4));
    CHECK(hipMalloc(&dsink, grid * 4));
    CHECK(hipMemcpy(dblk, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int hw = 0; hw < 2; ++hw) {
        std::vector<float> ms;
        for (int i = 0; i < 9; ++i) {
            CHECK(hipEventRecord(e0));
            if (hw) k_rate<1><<<grid, 256>>>(dblk, nblk, iters, dsink);
            else k_rate<0><<<grid, 256>>>(dblk, nblk, iters, dsink);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float t;
            CHECK(hipEventElapsedTime(&t, e0, e1));
            if (i >= 2) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        const double w = 16.0 * nblk * (double)iters * grid;
        printf("rate %-9s: median %.2f ms [%.2f .. %.2f], %.1f Gweights/s (decode only, cache-resident codes)\n", hw ? "hardware" : "integer", ms[3], ms.front(), ms.back(),
               w / ms[3] / 1e6);
    }
    return 0;
}
