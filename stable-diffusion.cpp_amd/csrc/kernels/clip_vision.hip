// clip_vision.hip — the two kernels in front of the CLIP vision tower (gfx950):
//   k_clip_preprocess  u8 HWC RGB pictures of any size -> pixel_values [S, S, 3, N] f32: value / 255, the nearest resize and the centre crop of the reference's
//                      clip_preprocess (src/core/util.cpp:695-758) as ONE gather through two host-built source-index tables, clamp to [0, 1], (v - mean) / std.
//                      Every operation is one rounded f32 operation, the divisions are IEEE divisions (no reciprocal), so the values are those of a NumPy restatement.
//   k_patch_embed      the whole CLIPVisionEmbeddings (src/model/te/clip.hpp:212-237) as one launch: the P x P stride-P conv as a GEMM over K = 3 P P, the class row,
//                      the position table.  As plain nodes: k_im2col, a generic GEMM, two transposing CONTs, a REPEAT, a CONCAT and an ADD.
//                        out[e, 1 + p, n] = sum_k W[k, e] * patch_k(p, n) + pos[e, 1 + p]        out[e, 0, n] = class[e] + pos[e, 0]
//                      One workgroup (4 waves) owns 64 patches x 64 embedding columns; wave w owns patch rows 16 w .. 16 w + 15 and all four 16-column tiles, one
//                      v_mfma_f32_16x16x32_f16 per tile and K step.  K is walked in chunks of 128 staged in LDS: the pixels converted to f16 in the pack (what the
//                      f16 im2col matrix of the plain route holds), the f16 weight rows copied; k >= K, patch rows behind the last patch and columns behind E are
//                      ZERO in LDS (K = 588 for P = 14 is no multiple of 32, K = 12 for P = 2 is less than one step).  LDS rows are 136 halfs (272 bytes): 16-byte
//                      aligned fragments, and the 16 rows of a fragment read start 4 banks apart.  f32 accumulation; the position row is added to the accumulator
//                      once, like the ADD node behind the conv.
#include "device_utils.h"
#include "kernels.h"
#include "ktime.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>

namespace mi355x {

static std::atomic<int64_t> g_patch_embed_launches;
int64_t patch_embed_launches() { return g_patch_embed_launches.load(std::memory_order_relaxed); }

// ---------------------------------------------------------------------------------------- preprocess
// img [N][h][w][3] u8; xi / yi: S source columns / rows; out [S, S, 3, N]
__global__ __launch_bounds__(256) void k_clip_preprocess(const uint8_t* __restrict__ img, const int* __restrict__ xi, const int* __restrict__ yi, float* __restrict__ out, int w, int h,
                                                           int S, int64_t total) {
#pragma clang fp contract(off)
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
    const float stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x     = (int)(i % S);
        const int y     = (int)((i / S) % S);
        const int c     = (int)((i / ((int64_t)S * S)) % 3);
        const int64_t n = i / ((int64_t)S * S * 3);
        float v         = (float)img[((n * h + yi[y]) * (int64_t)w + xi[x]) * 3 + c];
        v               = v / 255.0f;
        v               = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
        const float d   = v - mean[c];
        out[i]          = d / stdv[c];
    }
}

bool launch_clip_preprocess(hipStream_t s, const uint8_t* img, const int* xi, const int* yi, float* out, int w, int h, int S, int64_t n) {
    if (!img || !xi || !yi || !out || w < 1 || h < 1 || S < 1 || n < 1) return false;
    const int64_t total = (int64_t)S * S * 3 * n;
    KScope ks_(s, KF_OTHER, 0.0, (double)total * 5.0);
    const int64_t g = (total + 255) / 256;
    k_clip_preprocess<<<(int)(g > 4096 ? 4096 : g), 256, 0, s>>>(img, xi, yi, out, w, h, S, total);
    return true;
}

// ---------------------------------------------------------------------------------------- patch embedding
constexpr int PE_BM = 64, PE_BN = 64, PE_BK = 128, PE_LD = PE_BK + 8;

// x [S, S, 3, N] f32, w [K = 3 P P][E] f16 (ggml [P, P, 3, E]: k = kx + P (ky + P c) contiguous per e), cls [E], pos [E, np + 1], out [E, np + 1, N]; G = S / P, np = G G
__global__ __launch_bounds__(256) void k_patch_embed(const float* __restrict__ x, const _Float16* __restrict__ w, const float* __restrict__ cls, const float* __restrict__ pos,
                                                       float* __restrict__ out, int S, int P, int G, int E, int N) {
    __shared__ __attribute__((aligned(16))) _Float16 sa[PE_BM * PE_LD];
    __shared__ __attribute__((aligned(16))) _Float16 sb[PE_BN * PE_LD];
    const int np    = G * G;
    const int K     = 3 * P * P;
    const int rows  = N * np;  // patch rows of the GEMM, r = n * np + p
    const int e0    = blockIdx.x * PE_BN;
    const int r0    = blockIdx.y * PE_BM;
    const int tid   = threadIdx.x;
    const int lane  = tid & 63, wave = tid >> 6;
    const int PP    = P * P;

    // class row of this workgroup's columns, every image (the workgroups of the first patch tile only)
    if (blockIdx.y == 0) {
        for (int i = tid; i < PE_BN * N; i += 256) {
            const int e = e0 + (i % PE_BN), n = i / PE_BN;
            if (e < E) out[(int64_t)n * (np + 1) * E + e] = cls[e] + pos[e];
        }
    }

    float4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = float4_t{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < K; k0 += PE_BK) {
        __syncthreads();  // the previous chunk has been read
        for (int i = tid; i < PE_BM * PE_BK; i += 256) {
            const int kk = i % PE_BK, m = i / PE_BK;
            const int k = k0 + kk, r = r0 + m;
            float v = 0.f;
            if (k < K && r < rows) {
                const int n = r / np, p = r - n * np;
                const int py = p / G, px = p - py * G;
                const int c = k / PP, kr = k - c * PP;
                const int ky = kr / P, kx = kr - ky * P;
                v = x[(((int64_t)n * 3 + c) * S + (py * P + ky)) * S + (px * P + kx)];
            }
            sa[m * PE_LD + kk] = (_Float16)v;
        }
        for (int i = tid; i < PE_BN * PE_BK; i += 256) {
            const int kk = i % PE_BK, m = i / PE_BK;
            const int k = k0 + kk, e = e0 + m;
            sb[m * PE_LD + kk] = (k < K && e < E) ? w[(int64_t)e * K + k] : (_Float16)0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < PE_BK; ks += 32) {
            if (k0 + ks >= K) break;  // (uniform: the rest of the chunk is zero)
            // A[row = lane & 15][k = 8 (lane >> 4) + j], B[k = 8 (lane >> 4) + j][col = lane & 15]
            const half8_t a = *(const half8_t*)&sa[(wave * 16 + (lane & 15)) * PE_LD + ks + 8 * (lane >> 4)];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const half8_t b = *(const half8_t*)&sb[(t * 16 + (lane & 15)) * PE_LD + ks + 8 * (lane >> 4)];
                acc[t]          = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[t], 0, 0, 0);
            }
        }
    }
    // C / D: col = lane & 15 (embedding column), row = 4 (lane >> 4) + j (patch row)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int e = e0 + t * 16 + (lane & 15);
        if (e >= E) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = r0 + wave * 16 + 4 * (lane >> 4) + j;
            if (r >= rows) continue;
            const int n = r / np, p = r - n * np;
            out[((int64_t)n * (np + 1) + 1 + p) * E + e] = acc[t][j] + pos[(int64_t)(1 + p) * E + e];
        }
    }
}

bool patch_embed_shape_ok(int64_t S, int64_t P, int64_t E, int64_t N) {
    if (S < 1 || P < 1 || E < 1 || N < 1 || S % P != 0) return false;
    const int64_t G = S / P;
    // int indices inside the kernel; grid.y is a 16-bit dimension
    return S <= 4096 && P <= 64 && E <= (1 << 20) && N * G * G <= (int64_t)65535 * PE_BM && N * (G * G + 1) * E < ((int64_t)1 << 40) && N * 3 * S * S < ((int64_t)1 << 31);
}

void launch_patch_embed(hipStream_t s, float* out, const float* x, const void* w16, const float* cls, const float* pos, int64_t S, int64_t P, int64_t E, int64_t N) {
    if (!patch_embed_shape_ok(S, P, E, N)) {
        fprintf(stderr, "launch_patch_embed: unsupported shape S %lld P %lld E %lld N %lld\n", (long long)S, (long long)P, (long long)E, (long long)N);
        abort();
    }
    const int64_t G = S / P, rows = N * G * G, K = 3 * P * P;
    KScope ks_(s, KF_OTHER, 2.0 * (double)rows * (double)E * (double)K, (double)N * 3 * S * S * 4.0 + (double)E * K * 2.0 + (double)N * (G * G + 1) * E * 4.0);
    g_patch_embed_launches.fetch_add(1, std::memory_order_relaxed);
    const dim3 grid((unsigned)((E + PE_BN - 1) / PE_BN), (unsigned)((rows + PE_BM - 1) / PE_BM));
    k_patch_embed<<<grid, 256, 0, s>>>(x, (const _Float16*)w16, cls, pos, out, (int)S, (int)P, (int)G, (int)E, (int)N);
}

}  // namespace mi355x
