// elementwise.hip — HBM-bound glue kernels (gfx950): broadcast binary ops, unary activations, scale,
// strided copy/cast (+ LDS-tiled batched transpose fast path), concat, repeat, nearest upscale, pad,
// timestep embedding, GEGLU.  All are judged against the HBM roofline: algorithmic bytes = one read of
// each input + one write of the output.  128-bit accesses wherever the layout allows.
#include "kernels.h"
#include "ktime.h"
#include "device_utils.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>

namespace mi355x {

// launches per route (kernels.h EwRoute), for the statistics: one relaxed increment where a launcher has chosen its kernel
static std::atomic<int64_t> g_route_launches[EW_ROUTE_COUNT];
static inline void route_taken(EwRoute r) { g_route_launches[r].fetch_add(1, std::memory_order_relaxed); }
int64_t elementwise_route_launches(int route) { return route >= 0 && route < EW_ROUTE_COUNT ? g_route_launches[route].load(std::memory_order_relaxed) : 0; }

static inline double v4_elems(const View4& v) { return (double)v.ne[0] * (double)v.ne[1] * (double)v.ne[2] * (double)v.ne[3]; }
static inline double v4_esize(const View4& v) { return v.type == 0 ? 4.0 : (v.type == 1 || v.type == 30 ? 2.0 : 4.0); }


static inline int grid_for(int64_t n, int block, int cap = 256 * 16) {
    int64_t g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---------------------------------------------------------------------------------------- binary
template <int OP>
__device__ __forceinline__ float bin_apply(float x, float y) {
    if (OP == BIN_ADD) return x + y;
    if (OP == BIN_SUB) return x - y;
    if (OP == BIN_MUL) return x * y;
    return x / y;
}

// same-shape contiguous: float4
template <int OP>
__global__ void k_bin_same(float* __restrict__ dst, const float* __restrict__ a, const float* __restrict__ b, int64_t n4, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 x = ((const float4*)a)[i], y = ((const float4*)b)[i], r;
        r.x = bin_apply<OP>(x.x, y.x);
        r.y = bin_apply<OP>(x.y, y.y);
        r.z = bin_apply<OP>(x.z, y.z);
        r.w = bin_apply<OP>(x.w, y.w);
        ((float4*)dst)[i] = r;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        int64_t i = (n & ~3ll) + threadIdx.x;
        dst[i]    = bin_apply<OP>(a[i], b[i]);
    }
}
// b is a vector along ne0 (bias over tokens): a contiguous rows of ne0 (ne0 % 4 == 0)
template <int OP>
__global__ void k_bin_rowvec(float* __restrict__ dst, const float* __restrict__ a, const float* __restrict__ b, int64_t n4, int ne0_4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 x = ((const float4*)a)[i], y = ((const float4*)b)[i % ne0_4], r;
        r.x = bin_apply<OP>(x.x, y.x);
        r.y = bin_apply<OP>(x.y, y.y);
        r.z = bin_apply<OP>(x.z, y.z);
        r.w = bin_apply<OP>(x.w, y.w);
        ((float4*)dst)[i] = r;
    }
}
// b is one vector along ne0 PER IMAGE: a [C, L, N] contiguous, b [C, 1, N]
template <int OP>
__global__ void k_bin_tokvec(float* __restrict__ dst, const float* __restrict__ a, const float* __restrict__ b, int64_t n4, int ne0_4, int64_t img4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 x = ((const float4*)a)[i], y = ((const float4*)b)[(i / img4) * ne0_4 + i % ne0_4], r;
        r.x = bin_apply<OP>(x.x, y.x);
        r.y = bin_apply<OP>(x.y, y.y);
        r.z = bin_apply<OP>(x.z, y.z);
        r.w = bin_apply<OP>(x.w, y.w);
        ((float4*)dst)[i] = r;
    }
}
// b indexed by (i / inner) % bC + ((i / (inner*C)) % bN) * bC : per-channel (and per-image) scalar; inner % 4 == 0
template <int OP>
__global__ void k_bin_chan(float* __restrict__ dst, const float* __restrict__ a, const float* __restrict__ b, int64_t n4, int64_t inner4, int C,
                           int bN, int aN) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ch = i / inner4;
        const int c      = (int)(ch % C);
        const int nn     = (int)((ch / C) % aN) % bN;
        const float y    = b[(int64_t)nn * C + c];
        float4 x = ((const float4*)a)[i], r;
        r.x = bin_apply<OP>(x.x, y);
        r.y = bin_apply<OP>(x.y, y);
        r.z = bin_apply<OP>(x.z, y);
        r.w = bin_apply<OP>(x.w, y);
        ((float4*)dst)[i] = r;
    }
}
struct BinArgs {
    int64_t ne[4];
    int64_t anb[4], bnb[4], dnb[4];
    int64_t bne[4];
};
template <int OP>
__global__ void k_bin_generic(char* __restrict__ dst, const char* __restrict__ a, const char* __restrict__ b, BinArgs g, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = i % g.ne[0], i1 = (i / g.ne[0]) % g.ne[1], i2 = (i / (g.ne[0] * g.ne[1])) % g.ne[2], i3 = i / (g.ne[0] * g.ne[1] * g.ne[2]);
        const float x = *(const float*)(a + i0 * g.anb[0] + i1 * g.anb[1] + i2 * g.anb[2] + i3 * g.anb[3]);
        const float y = *(const float*)(b + (i0 % g.bne[0]) * g.bnb[0] + (i1 % g.bne[1]) * g.bnb[1] + (i2 % g.bne[2]) * g.bnb[2] + (i3 % g.bne[3]) * g.bnb[3]);
        *(float*)(dst + i0 * g.dnb[0] + i1 * g.dnb[1] + i2 * g.dnb[2] + i3 * g.dnb[3]) = bin_apply<OP>(x, y);
    }
}

static bool contig_f32(const int64_t ne[4], const int64_t nb[4]) {
    int64_t s = 4;
    for (int i = 0; i < 4; ++i) {
        if (ne[i] != 1 && nb[i] != s) return false;
        s *= ne[i];
    }
    return true;
}

template <int OP>
static void binary_dispatch(hipStream_t s, void* dst, const int64_t dnb[4], const View4& a, const View4& b) {
    const int64_t n   = a.ne[0] * a.ne[1] * a.ne[2] * a.ne[3];
    const bool ac     = contig_f32(a.ne, a.nb) && contig_f32(a.ne, dnb);
    const bool bc     = contig_f32(b.ne, b.nb);
    const bool al16   = (((uintptr_t)a.data | (uintptr_t)b.data | (uintptr_t)dst) & 15) == 0;
    const int block   = 256;
    if (ac && bc && al16) {
        const bool same = a.ne[0] == b.ne[0] && a.ne[1] == b.ne[1] && a.ne[2] == b.ne[2] && a.ne[3] == b.ne[3];
        if (same) {
            route_taken(EW_BIN_SAME);
            k_bin_same<OP><<<grid_for(n / 4 + 1, block), block, 0, s>>>((float*)dst, (const float*)a.data, (const float*)b.data, n / 4, n);
            return;
        }
        if (b.ne[0] == a.ne[0] && b.ne[1] == 1 && b.ne[2] == 1 && b.ne[3] == 1 && a.ne[0] % 4 == 0) {
            route_taken(EW_BIN_ROWVEC);
            k_bin_rowvec<OP><<<grid_for(n / 4, block), block, 0, s>>>((float*)dst, (const float*)a.data, (const float*)b.data, n / 4, (int)(a.ne[0] / 4));
            return;
        }
        // [C,1,N] broadcast over the tokens of [C,L,N] (adaLN modulate / gate of the DiT blocks, mmdit.hpp:368-380)
        if (b.ne[0] == a.ne[0] && b.ne[1] == 1 && a.ne[1] > 1 && b.ne[2] == a.ne[2] && b.ne[3] == 1 && a.ne[3] == 1 && a.ne[0] % 4 == 0) {
            route_taken(EW_BIN_TOKVEC);
            k_bin_tokvec<OP><<<grid_for(n / 4, block), block, 0, s>>>((float*)dst, (const float*)a.data, (const float*)b.data, n / 4, (int)(a.ne[0] / 4),
                                                                     a.ne[0] / 4 * a.ne[1]);
            return;
        }
        // [1,1,C,N'] broadcast over [W,H,C,N] (conv bias, group-norm affine, time-embedding add)
        const int64_t inner = a.ne[0] * a.ne[1];
        if (b.ne[0] == 1 && b.ne[1] == 1 && b.ne[2] == a.ne[2] && inner % 4 == 0 && (b.ne[3] == 1 || b.ne[3] == a.ne[3])) {
            route_taken(EW_BIN_CHAN);
            k_bin_chan<OP><<<grid_for(n / 4, block), block, 0, s>>>((float*)dst, (const float*)a.data, (const float*)b.data, n / 4, inner / 4,
                                                                   (int)a.ne[2], (int)b.ne[3], (int)a.ne[3]);
            return;
        }
    }
    BinArgs g;
    for (int i = 0; i < 4; ++i) {
        g.ne[i]  = a.ne[i];
        g.anb[i] = a.nb[i];
        g.bnb[i] = b.nb[i];
        g.dnb[i] = dnb[i];
        g.bne[i] = b.ne[i];
    }
    route_taken(EW_BIN_GENERIC);
    k_bin_generic<OP><<<grid_for(n, block), block, 0, s>>>((char*)dst, (const char*)a.data, (const char*)b.data, g, n);
}

void launch_binary(hipStream_t s, BinOp op, void* dst, const int64_t dnb[4], const View4& a, const View4& b) {
    KScope ks_(s, KF_BINARY, 0.0, v4_elems(a) * 8.0 + v4_elems(b) * 4.0);  // read a (+ broadcast b), write dst
    switch (op) {
        case BIN_ADD: binary_dispatch<BIN_ADD>(s, dst, dnb, a, b); break;
        case BIN_SUB: binary_dispatch<BIN_SUB>(s, dst, dnb, a, b); break;
        case BIN_MUL: binary_dispatch<BIN_MUL>(s, dst, dnb, a, b); break;
        default: binary_dispatch<BIN_DIV>(s, dst, dnb, a, b); break;
    }
}

// ---------------------------------------------------------------------------------------- VAE tile merge
// V = 4: every rectangle, the bounding box and every stride / offset are multiples of 4 cells and the pointers 16-byte aligned (decode: positions and skips are
// multiples of 8 pixels), so a float4 group lies inside or outside a tile as a whole; V = 1: arbitrary offsets (encode merges at latent resolution).
template <int V>
__global__ void k_tile_merge(float* __restrict__ canvas, const float* __restrict__ tiles, const float* __restrict__ wx, const float* __restrict__ wy,
                             const TileMergeArgs a) {
    // hipcc contracts a + b * c into one fused operation by default, and this toolchain's __fmul_rn / __fadd_rn are plain operators compiled under that default:
    // the pragma is what keeps the three roundings of old + ((new * s_y) * s_x) apart, so that the launch gives the bits of the MUL / MUL / ADD nodes it replaces
#pragma clang fp contract(off)
    const int bwv      = a.bw / V;
    const int64_t ntot = (int64_t)bwv * a.bh * a.planes;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ntot; i += (int64_t)gridDim.x * blockDim.x) {
        const int x       = a.bx + (int)(i % bwv) * V;
        const int y       = a.by + (int)((i / bwv) % a.bh);
        const int plane   = (int)(i / ((int64_t)bwv * a.bh));
        const int c       = plane % a.C, img = plane / a.C;
        float* cp         = canvas + (int64_t)img * a.c_img + (int64_t)c * a.c_plane + (int64_t)y * a.c_row + x;
        const int64_t sp  = (int64_t)img * a.s_img + (int64_t)c * a.s_plane;
        float acc[V];
        bool covered = false, loaded = false;
        for (int t = 0; t < a.k; ++t) {
            const TileMergeTile& d = a.t[t];
            const int tx = x - d.x, ty = y - d.y;
            if (tx < 0 || ty < 0 || tx >= d.w || ty >= d.h) continue;
            if (!a.store && !loaded) {
                if constexpr (V == 4) {
                    const float4 o = *(const float4*)cp;
                    acc[0] = o.x, acc[1] = o.y, acc[2] = o.z, acc[3] = o.w;
                } else {
                    acc[0] = *cp;
                }
                loaded = true;
            }
            covered            = true;
            const float* src   = tiles + d.src + sp + (int64_t)ty * a.s_row + tx;
            const float fy     = wy[d.wy + ty];
            float v[V], fx[V];
            if constexpr (V == 4) {
                const float4 q = *(const float4*)src, r = *(const float4*)(wx + d.wx + tx);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                fx[0] = r.x, fx[1] = r.y, fx[2] = r.z, fx[3] = r.w;
            } else {
                v[0]  = *src;
                fx[0] = wx[d.wx + tx];
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float m = (v[e] * fy) * fx[e];  // plain operators: they take this function's contraction state (the header's __fmul_rn / __fadd_rn carry their own)
                acc[e]        = a.store ? m : acc[e] + m;
            }
        }
        if (!covered) continue;
        if constexpr (V == 4)
            *(float4*)cp = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else
            *cp = acc[0];
    }
}

void launch_tile_merge(hipStream_t s, float* canvas, const float* tiles, const float* wx, const float* wy, const TileMergeArgs& a) {
    double cells = 0;
    bool v4      = ((((uintptr_t)canvas | (uintptr_t)tiles | (uintptr_t)wx) & 15) == 0) && a.bx % 4 == 0 && a.bw % 4 == 0 && a.c_row % 4 == 0 && a.c_plane % 4 == 0 &&
              a.c_img % 4 == 0 && a.s_row % 4 == 0 && a.s_plane % 4 == 0 && a.s_img % 4 == 0;
    for (int t = 0; t < a.k; ++t) {
        const TileMergeTile& d = a.t[t];
        cells += (double)d.w * d.h;
        v4 = v4 && d.x % 4 == 0 && d.w % 4 == 0 && d.src % 4 == 0 && d.wx % 4 == 0;
    }
    KScope ks_(s, KF_BINARY, 0.0, cells * a.planes * 4.0 + (double)a.bw * a.bh * a.planes * 8.0);  // read every tile cell once, read + write the box of the canvas
    const int64_t n = (int64_t)(a.bw / (v4 ? 4 : 1)) * a.bh * a.planes;
    if (n <= 0) return;
    route_taken(v4 ? EW_TILE_MERGE_V4 : EW_TILE_MERGE_V1);
    if (v4)
        k_tile_merge<4><<<grid_for(n, 256), 256, 0, s>>>(canvas, tiles, wx, wy, a);
    else
        k_tile_merge<1><<<grid_for(n, 256), 256, 0, s>>>(canvas, tiles, wx, wy, a);
}

// ---------------------------------------------------------------------------------------- unary
template <int OP>
__global__ void k_unary(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
    const int64_t n4 = n / 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 x = ((const float4*)src)[i], r;
        r.x = act_apply<OP>(x.x);
        r.y = act_apply<OP>(x.y);
        r.z = act_apply<OP>(x.z);
        r.w = act_apply<OP>(x.w);
        ((float4*)dst)[i] = r;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        int64_t i = (n & ~3ll) + threadIdx.x;
        dst[i]    = act_apply<OP>(src[i]);
    }
}
void launch_unary(hipStream_t s, UnOp op, float* dst, const float* src, int64_t n) {
    KScope ks_(s, KF_UNARY, 0.0, (double)n * 8.0);
    const int block = 256, grid = grid_for(n / 4 + 1, block);
#define U(OPV) case OPV: k_unary<OPV><<<grid, block, 0, s>>>(dst, src, n); break;
    switch (op) {
        U(UN_SILU) U(UN_GELU) U(UN_GELU_QUICK) U(UN_SIGMOID) U(UN_TANH) U(UN_RELU) U(UN_NEG) U(UN_EXP) U(UN_GELU_ERF)
    }
#undef U
}

__global__ void k_scale(float* __restrict__ dst, const float* __restrict__ src, int64_t n, float sc, float bias) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i] * sc + bias;
}
void launch_scale(hipStream_t s, float* dst, const float* src, int64_t n, float scale, float bias) {
    KScope ks_(s, KF_UNARY, 0.0, (double)n * 8.0);
    k_scale<<<grid_for(n, 256), 256, 0, s>>>(dst, src, n, scale, bias);
}

// ---------------------------------------------------------------------------------------- copy / cast
struct CopyArgs {
    int64_t sne[4], snb[4], dne[4], dnb[4];
};
template <typename TS, typename TD>
__global__ void k_copy_generic(char* __restrict__ dst, const char* __restrict__ src, CopyArgs g, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a0 = i % g.sne[0], a1 = (i / g.sne[0]) % g.sne[1], a2 = (i / (g.sne[0] * g.sne[1])) % g.sne[2], a3 = i / (g.sne[0] * g.sne[1] * g.sne[2]);
        const int64_t b0 = i % g.dne[0], b1 = (i / g.dne[0]) % g.dne[1], b2 = (i / (g.dne[0] * g.dne[1])) % g.dne[2], b3 = i / (g.dne[0] * g.dne[1] * g.dne[2]);
        const TS v = *(const TS*)(src + a0 * g.snb[0] + a1 * g.snb[1] + a2 * g.snb[2] + a3 * g.snb[3]);
        *(TD*)(dst + b0 * g.dnb[0] + b1 * g.dnb[1] + b2 * g.dnb[2] + b3 * g.dnb[3]) = cvt<TD>(v);
    }
}
// same logical shape, ne0 contiguous on both sides (permuted / sliced rows: split_qkv, head permutes, chunk, slice): 4 elements per thread
template <typename TS, typename TD>
__global__ void k_copy_rows(char* __restrict__ dst, const char* __restrict__ src, CopyArgs g, int64_t n4) {
    const int64_t r0 = g.sne[0] / 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i % r0, row = i / r0;
        const int64_t i1 = row % g.sne[1], t = row / g.sne[1], i2 = t % g.sne[2], i3 = t / g.sne[2];
        TS v[4];
        *(vec_t<TS, 4>*)v = *(const vec_t<TS, 4>*)(src + i1 * g.snb[1] + i2 * g.snb[2] + i3 * g.snb[3] + c * 4 * (int64_t)sizeof(TS));
        TD r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = cvt<TD>(v[j]);
        *(vec_t<TD, 4>*)(dst + i1 * g.dnb[1] + i2 * g.dnb[2] + i3 * g.dnb[3] + c * 4 * (int64_t)sizeof(TD)) = *(vec_t<TD, 4>*)r;
    }
}
// contiguous -> contiguous with conversion, 4 elements per thread
template <typename TS, typename TD>
__global__ void k_copy_contig(TD* __restrict__ dst, const TS* __restrict__ src, int64_t n) {
    const int64_t n4 = n / 4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        TS v[4];
        *(vec_t<TS, 4>*)v = ((const vec_t<TS, 4>*)src)[i];
        TD r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = cvt<TD>(v[j]);
        ((vec_t<TD, 4>*)dst)[i] = *(vec_t<TD, 4>*)r;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        int64_t i = (n & ~3ll) + threadIdx.x;
        dst[i]    = cvt<TD>(src[i]);
    }
}
// batched 2-D transpose through LDS: dst[b][r][c] (c contiguous) = src[b][c][r] (r contiguous in src)
// i.e. src element (r, c) at src + r*1 + c*src_ld ; dst element at dst + c + r*dst_ld   (in elements)
template <typename TS, typename TD>
__global__ void k_transpose(TD* __restrict__ dst, const TS* __restrict__ src, int R, int Cc, int64_t src_ld, int64_t dst_ld,
                            int64_t src_bs, int64_t dst_bs, int nb1, int64_t src_bs2, int64_t dst_bs2) {
    __shared__ float tile[64][65];
    const int b  = blockIdx.z;
    const int b1 = b % nb1, b2 = b / nb1;
    src += b1 * src_bs + b2 * src_bs2;
    dst += b1 * dst_bs + b2 * dst_bs2;
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 256 threads: 64 x 4
    for (int j = ty; j < 64; j += 4) {
        const int r = r0 + tx, c = c0 + j;
        if (r < R && c < Cc) tile[j][tx] = to_f32(src[(int64_t)c * src_ld + r]);
    }
    __syncthreads();
    for (int j = ty; j < 64; j += 4) {
        const int c = c0 + tx, r = r0 + j;
        if (r < R && c < Cc) dst[(int64_t)r * dst_ld + c] = cvt<TD>(tile[tx][j]);
    }
}

template <typename TS, typename TD>
static void copy_typed(hipStream_t s, const View4& dst, const View4& src) {
    const int64_t n = src.ne[0] * src.ne[1] * src.ne[2] * src.ne[3];
    auto contig = [](const View4& v, int64_t es) {
        int64_t st = es;
        for (int i = 0; i < 4; ++i) {
            if (v.ne[i] != 1 && v.nb[i] != st) return false;
            st *= v.ne[i];
        }
        return true;
    };
    const bool dc = contig(dst, sizeof(TD)), sc = contig(src, sizeof(TS));
    if (dc && sc && (((uintptr_t)dst.data | (uintptr_t)src.data) & 15) == 0) {
        route_taken(EW_COPY_CONTIG);
        k_copy_contig<TS, TD><<<grid_for(n / 4 + 1, 256), 256, 0, s>>>((TD*)dst.data, (const TS*)src.data, n);
        return;
    }
    // transpose fast path: same logical shape, dst contiguous, src a permuted view whose dim 1 is the
    // memory-contiguous one: batched 2-D transposes dst[.., r, c] = src[r + c*ld] staged through LDS.
    bool same = true;
    for (int i = 0; i < 4; ++i) same = same && (dst.ne[i] == src.ne[i]);
    if (same && dc && src.nb[0] != (int64_t)sizeof(TS) && src.nb[1] == (int64_t)sizeof(TS) && src.nb[0] % sizeof(TS) == 0 &&
        src.nb[2] % sizeof(TS) == 0 && src.nb[3] % sizeof(TS) == 0) {
        int64_t R = src.ne[1], nb1 = src.ne[2], sbs = src.nb[2], dbs = dst.nb[2];
        if (src.nb[2] == src.nb[1] * src.ne[1]) {  // dims 1,2 are one contiguous run in src (NCHW -> token-major)
            R *= src.ne[2];
            nb1 = 1;
            sbs = 0;
            dbs = 0;
        }
        if (nb1 * src.ne[3] <= 65535) {  // grid.z carries the batch: beyond its limit the launch would fail, the generic route below takes the copy
            const int Cc = (int)src.ne[0];
            dim3 grid((unsigned)((R + 63) / 64), (unsigned)((Cc + 63) / 64), (unsigned)(nb1 * src.ne[3]));
            route_taken(EW_COPY_TRANSPOSE);
            k_transpose<TS, TD><<<grid, 256, 0, s>>>((TD*)dst.data, (const TS*)src.data, (int)R, Cc, src.nb[0] / sizeof(TS), Cc,
                                                      sbs / sizeof(TS), dbs / sizeof(TD), (int)nb1, src.nb[3] / sizeof(TS), dst.nb[3] / sizeof(TD));
            return;
        }
    }
    CopyArgs g;
    for (int i = 0; i < 4; ++i) {
        g.sne[i] = src.ne[i];
        g.snb[i] = src.nb[i];
        g.dne[i] = dst.ne[i];
        g.dnb[i] = dst.nb[i];
    }
    {
        const int64_t sa = 4 * sizeof(TS), da = 4 * sizeof(TD);  // vector alignment in bytes
        bool rows = same && src.nb[0] == (int64_t)sizeof(TS) && dst.nb[0] == (int64_t)sizeof(TD) && src.ne[0] % 4 == 0 && ((uintptr_t)src.data % sa) == 0 &&
                    ((uintptr_t)dst.data % da) == 0;
        for (int i = 1; i < 4; ++i) rows = rows && src.nb[i] % sa == 0 && dst.nb[i] % da == 0;
        if (rows) {
            route_taken(EW_COPY_ROWS);
            k_copy_rows<TS, TD><<<grid_for(n / 4, 256), 256, 0, s>>>((char*)dst.data, (const char*)src.data, g, n / 4);
            return;
        }
    }
    route_taken(EW_COPY_GENERIC);
    k_copy_generic<TS, TD><<<grid_for(n, 256), 256, 0, s>>>((char*)dst.data, (const char*)src.data, g, n);
}

void launch_copy(hipStream_t s, const View4& dst, const View4& src) {
    KScope ks_(s, KF_COPY, 0.0, v4_elems(src) * (v4_esize(src) + v4_esize(dst)));
    const int F32 = 0, F16 = 1, BF16 = 30;
    if (src.type == F32 && dst.type == F32) return copy_typed<float, float>(s, dst, src);
    if (src.type == F32 && dst.type == F16) return copy_typed<float, __half>(s, dst, src);
    if (src.type == F16 && dst.type == F32) return copy_typed<__half, float>(s, dst, src);
    if (src.type == F16 && dst.type == F16) return copy_typed<__half, __half>(s, dst, src);
    if (src.type == F32 && dst.type == BF16) return copy_typed<float, bf16_t>(s, dst, src);
    if (src.type == BF16 && dst.type == F32) return copy_typed<bf16_t, float>(s, dst, src);
    fprintf(stderr, "[ggml-mi355x] launch_copy: unsupported type pair %d -> %d (planner_supports_op admits f32/f16 <-> f32/f16 and f32 <-> bf16)\n", src.type, dst.type);
    abort();
}

// ---------------------------------------------------------------------------------------- rotary embedding (interleaved pairs)
// Rope::apply_rope (src/model/common/rope.hpp:966-1004) as ONE kernel instead of its 8-node cont/repeat/mul/add chain:
//   x   [d, H, L, N] f32, any strides with d contiguous (a slice of a fused qkv projection, or a concat result)
//   pe  [2, 2, d/2, L] f32 contiguous: per token and pair the matrix [[cos, -sin], [sin, cos]]
//   out [d, L, H*N] f32 contiguous:  out[2j] = x[2j]*pe[0][0] + x[2j+1]*pe[0][1],  out[2j+1] = x[2j]*pe[1][0] + x[2j+1]*pe[1][1]
__global__ void k_rope_pairs(float* __restrict__ out, const char* __restrict__ x, const float* __restrict__ pe, int d2, int H, int64_t L, int64_t N, int64_t xnb1,
                             int64_t xnb2, int64_t xnb3, int64_t npairs) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * blockDim.x) {
        const int j     = (int)(i % d2);
        const int64_t t = i / d2, l = t % L, hn = t / L;
        const int64_t h = hn % H, n = hn / H;
        const float2 v  = *(const float2*)(x + h * xnb1 + l * xnb2 + n * xnb3 + (int64_t)j * 8);
        const float4 m  = *(const float4*)(pe + (l * d2 + j) * 4);  // (m00, m01, m10, m11) = (cos, -sin, sin, cos)
        float2 r;
        r.x = v.x * m.x + v.y * m.y;
        r.y = v.x * m.z + v.y * m.w;
        *(float2*)(out + ((hn * L + l) * d2 + j) * 2) = r;
    }
}
void launch_rope_pairs(hipStream_t s, float* out, const View4& x, const float* pe) {
    KScope ks_(s, KF_OTHER, 0.0, v4_elems(x) * 8.0);
    const int d2 = (int)(x.ne[0] / 2);
    const int64_t npairs = (int64_t)d2 * x.ne[1] * x.ne[2] * x.ne[3];
    k_rope_pairs<<<grid_for(npairs, 256), 256, 0, s>>>(out, (const char*)x.data, pe, d2, (int)x.ne[1], x.ne[2], x.ne[3], x.nb[1], x.nb[2], x.nb[3], npairs);
}

// ---------------------------------------------------------------------------------------- token concat straight into the attention operand
// MMDiT block_mixing (mmdit.hpp:640-646) + ggml_ext_attention_ext (ggml_extend.hpp:1366-1412): concat(ctx, x) along tokens -> reshape
// [d,H,Lt,N] -> permute(0,2,1,3) -> cont (-> cast f16) as ONE pass: out[dd, l, h, n] = (l < La ? a : b)[h*d + dd, l', n]
template <typename TD>
__global__ void k_concat_heads(TD* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b, int d4, int H, int64_t La, int64_t Lb, int64_t N,
                               int64_t n4) {
    const int64_t Lt = La + Lb, C4 = (int64_t)d4 * H;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int j      = (int)(i % d4);
        const int64_t t1 = i / d4, l = t1 % Lt, t2 = t1 / Lt, h = t2 % H, n = t2 / H;
        const float4 v   = l < La ? ((const float4*)a)[(n * La + l) * C4 + h * d4 + j] : ((const float4*)b)[(n * Lb + (l - La)) * C4 + h * d4 + j];
        TD r[4] = {cvt<TD>(v.x), cvt<TD>(v.y), cvt<TD>(v.z), cvt<TD>(v.w)};
        ((vec_t<TD, 4>*)out)[i] = *(vec_t<TD, 4>*)r;
    }
}
void launch_concat_heads(hipStream_t s, void* out, bool out_f16, const float* a, const float* b, int64_t d, int64_t H, int64_t La, int64_t Lb, int64_t N) {
    KScope ks_(s, KF_CONCAT, 0.0, (double)d * H * (La + Lb) * N * (4.0 + (out_f16 ? 2.0 : 4.0)));
    const int64_t n4 = d / 4 * H * (La + Lb) * N;
    if (out_f16)
        k_concat_heads<__half><<<grid_for(n4, 256), 256, 0, s>>>((__half*)out, a, b, (int)(d / 4), (int)H, La, Lb, N, n4);
    else
        k_concat_heads<float><<<grid_for(n4, 256), 256, 0, s>>>((float*)out, a, b, (int)(d / 4), (int)H, La, Lb, N, n4);
}

// joint-attention operand assembly (MMDiT: DitSelfAttention::pre_attention mmdit.hpp:299-366 + block_mixing :614-668 + ggml_ext_attention_ext):
// for ONE of q / k / v of both streams: the stream's columns of its fused qkv projection [rows][xs] -> per-head RMSNorm * w (q / k with qk-norm;
// w == nullptr: none) -> token concat (context rows first) -> head-major [d, Lt, H, N] as f32 or f16.  Replaces split_qkv's permuted copy, the
// strided norms, their weight MULs and the concat / permute / cast passes.  G lanes per head (d = 4 G), a head's 4 G floats are one contiguous run.
template <typename TD, int G>
__global__ void k_joint_heads(TD* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b, int64_t xsa, int64_t xsb, const float* __restrict__ wa,
                              const float* __restrict__ wb, float eps, int H, int64_t La, int64_t Lb, int64_t ngroups, const float* __restrict__ pe) {
    const int j      = threadIdx.x % G;
    const int64_t Lt = La + Lb;
    for (int64_t gi = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / G; gi < ngroups; gi += (int64_t)gridDim.x * blockDim.x / G) {
        const int h     = (int)(gi % H);
        const int64_t t = gi / H, l = t % Lt, n = t / Lt;
        const bool fst  = l < La;
        const float* src = fst ? a + (n * La + l) * xsa : b + (n * Lb + (l - La)) * xsb;  // (Lb == 0: one stream, b is never read)
        float4 v         = *(const float4*)(src + h * (4 * G) + 4 * j);
        const float* w   = fst ? wa : wb;
        if (w) {
            float ss = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
#pragma unroll
            for (int m = G / 2; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, G);
            const float sc  = 1.0f / sqrtf(ss / (float)(4 * G) + eps);
            const float4 ww = ((const float4*)w)[j];
            v.x = v.x * sc * ww.x; v.y = v.y * sc * ww.y; v.z = v.z * sc * ww.z; v.w = v.w * sc * ww.w;
        }
        if (pe) {  // rotary embedding of the pairs (4j, 4j+1), (4j+2, 4j+3) at joint position l: Rope::apply_rope (rope.hpp:966-1004), pe [2,2,d/2,Lt]
            const float4 m0 = *(const float4*)(pe + (l * (2 * G) + 2 * j) * 4), m1 = *(const float4*)(pe + (l * (2 * G) + 2 * j + 1) * 4);
            const float4 u  = v;
            v.x = u.x * m0.x + u.y * m0.y;
            v.y = u.x * m0.z + u.y * m0.w;
            v.z = u.z * m1.x + u.w * m1.y;
            v.w = u.z * m1.z + u.w * m1.w;
        }
        TD r[4] = {cvt<TD>(v.x), cvt<TD>(v.y), cvt<TD>(v.z), cvt<TD>(v.w)};
        ((vec_t<TD, 4>*)out)[((n * H + h) * Lt + l) * G + j] = *(vec_t<TD, 4>*)r;
    }
}
bool joint_heads_supported(int64_t d) { return d == 64 || d == 128; }
void launch_joint_heads(hipStream_t s, void* out, bool out_f16, const float* a, int64_t xsa, const float* wa, const float* b, int64_t xsb, const float* wb, float eps,
                        int64_t d, int64_t H, int64_t La, int64_t Lb, int64_t N, const float* pe) {
    KScope ks_(s, KF_CONCAT, 0.0, (double)d * H * (La + Lb) * N * (4.0 + (out_f16 ? 2.0 : 4.0)));
    const int64_t ng = H * (La + Lb) * N, nthr = ng * (d / 4);
    const unsigned grid = grid_for(nthr, 256);
#define JH(TD_, G_) k_joint_heads<TD_, G_><<<grid, 256, 0, s>>>((TD_*)out, a, b, xsa, xsb, wa, wb, eps, (int)H, La, Lb, ng, pe)
    if (d == 64) {
        if (out_f16) JH(__half, 16); else JH(float, 16);
    } else {
        if (out_f16) JH(__half, 32); else JH(float, 32);
    }
#undef JH
}

// ---------------------------------------------------------------------------------------- concat / repeat / upscale / pad
struct Idx4 {
    int64_t ne[4], nb[4];
};
__global__ void k_concat(char* __restrict__ dst, const char* __restrict__ a, const char* __restrict__ b, Idx4 d, Idx4 ga, Idx4 gb, int dim, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t idx[4] = {i % d.ne[0], (i / d.ne[0]) % d.ne[1], (i / (d.ne[0] * d.ne[1])) % d.ne[2], i / (d.ne[0] * d.ne[1] * d.ne[2])};
        char* dp       = dst + idx[0] * d.nb[0] + idx[1] * d.nb[1] + idx[2] * d.nb[2] + idx[3] * d.nb[3];
        const char* sp;
        if (idx[dim] < ga.ne[dim]) {
            sp = a + idx[0] * ga.nb[0] + idx[1] * ga.nb[1] + idx[2] * ga.nb[2] + idx[3] * ga.nb[3];
        } else {
            idx[dim] -= ga.ne[dim];
            sp = b + idx[0] * gb.nb[0] + idx[1] * gb.nb[1] + idx[2] * gb.nb[2] + idx[3] * gb.nb[3];
        }
        *(float*)dp = *(const float*)sp;
    }
}
// contiguous concat along dim 2 ([W,H,C,N]): per image, copy two contiguous slabs (float4)
__global__ void k_concat_dim2(float4* __restrict__ dst, const float4* __restrict__ a, const float4* __restrict__ b, int64_t sa4, int64_t sb4, int64_t n4) {
    const int64_t per = sa4 + sb4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t img = i / per, r = i % per;
        dst[i] = r < sa4 ? a[img * sa4 + r] : b[img * sb4 + (r - sa4)];
    }
}
// concat along dim 2 of [ne0, ne1, L, N] tensors whose (ne0, ne1) plane is contiguous in a, b and dst (per-head q/k/v of the txt and img
// streams, flux.hpp:540-544: v is a strided slice of the fused qkv projection): whole planes are copied as float4 runs
__global__ void k_concat_planes(float4* __restrict__ dst, const char* __restrict__ a, const char* __restrict__ b, int64_t plane4, int64_t La, int64_t Lb,
                                int64_t a_nb2, int64_t a_nb3, int64_t b_nb2, int64_t b_nb3, int64_t n4) {
    const int64_t Lt = La + Lb;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = i % plane4, t = i / plane4, l = t % Lt, n = t / Lt;
        const char* src = l < La ? a + l * a_nb2 + n * a_nb3 : b + (l - La) * b_nb2 + n * b_nb3;
        dst[i]          = ((const float4*)src)[c];
    }
}
static Idx4 mk(const View4& v) {
    Idx4 r;
    for (int i = 0; i < 4; ++i) {
        r.ne[i] = v.ne[i];
        r.nb[i] = v.nb[i];
    }
    return r;
}
void launch_concat(hipStream_t s, const View4& dst, const View4& a, const View4& b, int dim) {
    KScope ks_(s, KF_CONCAT, 0.0, v4_elems(dst) * 8.0);
    const int64_t n = dst.ne[0] * dst.ne[1] * dst.ne[2] * dst.ne[3];
    if (dim == 2 && contig_f32(a.ne, a.nb) && contig_f32(b.ne, b.nb) && contig_f32(dst.ne, dst.nb)) {
        const int64_t sa = a.ne[0] * a.ne[1] * a.ne[2], sb = b.ne[0] * b.ne[1] * b.ne[2];
        if (sa % 4 == 0 && sb % 4 == 0 && (((uintptr_t)a.data | (uintptr_t)b.data | (uintptr_t)dst.data) & 15) == 0) {
            route_taken(EW_CONCAT_DIM2);
            k_concat_dim2<<<grid_for(n / 4, 256), 256, 0, s>>>((float4*)dst.data, (const float4*)a.data, (const float4*)b.data, sa / 4, sb / 4, n / 4);
            return;
        }
    }
    if (dim == 2 && contig_f32(dst.ne, dst.nb)) {
        const int64_t plane = dst.ne[0] * dst.ne[1];
        auto plane_ok = [&](const View4& v) {
            return v.nb[0] == 4 && (v.ne[1] == 1 || v.nb[1] == v.ne[0] * 4) && v.nb[2] % 16 == 0 && v.nb[3] % 16 == 0 && (((uintptr_t)v.data) & 15) == 0;
        };
        if (plane % 4 == 0 && plane_ok(a) && plane_ok(b) && (((uintptr_t)dst.data) & 15) == 0) {
            route_taken(EW_CONCAT_PLANES);
            k_concat_planes<<<grid_for(n / 4, 256), 256, 0, s>>>((float4*)dst.data, (const char*)a.data, (const char*)b.data, plane / 4, a.ne[2], b.ne[2], a.nb[2], a.nb[3],
                                                                b.nb[2], b.nb[3], n / 4);
            return;
        }
    }
    route_taken(EW_CONCAT_GENERIC);
    k_concat<<<grid_for(n, 256), 256, 0, s>>>((char*)dst.data, (const char*)a.data, (const char*)b.data, mk(dst), mk(a), mk(b), dim, n);
}

__global__ void k_repeat(char* __restrict__ dst, const char* __restrict__ src, Idx4 d, Idx4 g, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = i % d.ne[0], i1 = (i / d.ne[0]) % d.ne[1], i2 = (i / (d.ne[0] * d.ne[1])) % d.ne[2], i3 = i / (d.ne[0] * d.ne[1] * d.ne[2]);
        *(float*)(dst + i0 * d.nb[0] + i1 * d.nb[1] + i2 * d.nb[2] + i3 * d.nb[3]) =
            *(const float*)(src + (i0 % g.ne[0]) * g.nb[0] + (i1 % g.ne[1]) * g.nb[1] + (i2 % g.ne[2]) * g.nb[2] + (i3 % g.ne[3]) * g.nb[3]);
    }
}
void launch_repeat(hipStream_t s, const View4& dst, const View4& src) {
    KScope ks_(s, KF_COPY, 0.0, v4_elems(dst) * 4.0 + v4_elems(src) * 4.0);
    const int64_t n = dst.ne[0] * dst.ne[1] * dst.ne[2] * dst.ne[3];
    k_repeat<<<grid_for(n, 256), 256, 0, s>>>((char*)dst.data, (const char*)src.data, mk(dst), mk(src), n);
}

__global__ void k_upscale(char* __restrict__ dst, const char* __restrict__ src, Idx4 d, Idx4 g, float sf0, float sf1, float sf2, float sf3, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = i % d.ne[0], i1 = (i / d.ne[0]) % d.ne[1], i2 = (i / (d.ne[0] * d.ne[1])) % d.ne[2], i3 = i / (d.ne[0] * d.ne[1] * d.ne[2]);
        const int64_t j0 = (int64_t)(i0 / sf0), j1 = (int64_t)(i1 / sf1), j2 = (int64_t)(i2 / sf2), j3 = (int64_t)(i3 / sf3);
        *(float*)(dst + i0 * d.nb[0] + i1 * d.nb[1] + i2 * d.nb[2] + i3 * d.nb[3]) = *(const float*)(src + j0 * g.nb[0] + j1 * g.nb[1] + j2 * g.nb[2] + j3 * g.nb[3]);
    }
}
void launch_upscale_nearest(hipStream_t s, const View4& dst, const View4& src) {
    KScope ks_(s, KF_COPY, 0.0, v4_elems(dst) * 4.0 + v4_elems(src) * 4.0);
    const int64_t n = dst.ne[0] * dst.ne[1] * dst.ne[2] * dst.ne[3];
    k_upscale<<<grid_for(n, 256), 256, 0, s>>>((char*)dst.data, (const char*)src.data, mk(dst), mk(src), (float)dst.ne[0] / src.ne[0],
                                              (float)dst.ne[1] / src.ne[1], (float)dst.ne[2] / src.ne[2], (float)dst.ne[3] / src.ne[3], n);
}

struct Pads {
    int32_t p[8];
};
__global__ void k_pad(char* __restrict__ dst, const char* __restrict__ src, Idx4 d, Idx4 g, Pads pd, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i0 = i % d.ne[0], i1 = (i / d.ne[0]) % d.ne[1], i2 = (i / (d.ne[0] * d.ne[1])) % d.ne[2], i3 = i / (d.ne[0] * d.ne[1] * d.ne[2]);
        const int64_t j0 = i0 - pd.p[0], j1 = i1 - pd.p[2], j2 = i2 - pd.p[4], j3 = i3 - pd.p[6];
        float v = 0.f;
        if (j0 >= 0 && j0 < g.ne[0] && j1 >= 0 && j1 < g.ne[1] && j2 >= 0 && j2 < g.ne[2] && j3 >= 0 && j3 < g.ne[3])
            v = *(const float*)(src + j0 * g.nb[0] + j1 * g.nb[1] + j2 * g.nb[2] + j3 * g.nb[3]);
        *(float*)(dst + i0 * d.nb[0] + i1 * d.nb[1] + i2 * d.nb[2] + i3 * d.nb[3]) = v;
    }
}
void launch_pad(hipStream_t s, const View4& dst, const View4& src, const int32_t pads[8]) {
    const int64_t n = dst.ne[0] * dst.ne[1] * dst.ne[2] * dst.ne[3];
    Pads pd;
    for (int i = 0; i < 8; ++i) pd.p[i] = pads[i];
    k_pad<<<grid_for(n, 256), 256, 0, s>>>((char*)dst.data, (const char*)src.data, mk(dst), mk(src), pd, n);
}

// ---------------------------------------------------------------------------------------- timestep embedding
// dst[j]=cos(t*f_j), dst[j+half]=sin(t*f_j), f_j=exp(-ln(max_period)*j/half)   (ggml_extend.hpp:1579-1606)
__global__ void k_timestep_embedding(float* __restrict__ dst, const float* __restrict__ t, int dim, int max_period, int64_t row_stride) {
    const int i    = blockIdx.x;
    const int half = dim / 2;
    float* emb     = dst + i * row_stride;
    const float ts = t[i];
    for (int j = threadIdx.x; j < half; j += blockDim.x) {
        const float freq = expf(-logf((float)max_period) * j / half);
        const float arg  = ts * freq;
        emb[j]           = cosf(arg);
        emb[j + half]    = sinf(arg);
    }
    if ((dim & 1) && threadIdx.x == 0) emb[2 * half] = 0.f;
}
void launch_timestep_embedding(hipStream_t s, float* dst, const float* t, int n, int dim, int max_period, int64_t dst_row_stride) {
    k_timestep_embedding<<<n, 128, 0, s>>>(dst, t, dim, max_period, dst_row_stride);
}

// ---------------------------------------------------------------------------------------- GEGLU
__global__ void k_geglu(float* __restrict__ dst, const float* __restrict__ x, int64_t n4, int inner4, int64_t x_stride4) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = i / inner4;
        const int c     = (int)(i % inner4);
        const float4 a = ((const float4*)x)[t * x_stride4 + c], g = ((const float4*)x)[t * x_stride4 + inner4 + c];
        float4 r;
        r.x = a.x * act_apply<UN_GELU>(g.x);
        r.y = a.y * act_apply<UN_GELU>(g.y);
        r.z = a.z * act_apply<UN_GELU>(g.z);
        r.w = a.w * act_apply<UN_GELU>(g.w);
        ((float4*)dst)[i] = r;
    }
}
void launch_geglu(hipStream_t s, float* dst, const float* x, int64_t tokens, int64_t inner, int64_t x_stride) {
    KScope ks_(s, KF_OTHER, 0.0, (double)tokens * inner * 12.0);
    const int64_t n4 = tokens * inner / 4;
    k_geglu<<<grid_for(n4, 256), 256, 0, s>>>(dst, x, n4, (int)(inner / 4), x_stride / 4);
}

// ---------------------------------------------------------------------------------------- GET_ROWS (embedding gather)
// dst[:, i10, i11, i12] = dequant(table[ids[i10, i11, i12], :] of plane (i11, i12)); one workgroup per gathered row.  HBM-bound:
// nc * (table element + 4) bytes per row.  f32 / f16 / bf16 tables and ggml's q8_0 / q4_0 blocks.
template <int TYPE>
__global__ void k_get_rows(float* __restrict__ dst, const char* __restrict__ table, const char* __restrict__ ids, int64_t nc, int64_t ne10, int64_t ne11,
                           int64_t ib0, int64_t ib1, int64_t ib2, int64_t tb1, int64_t tb2, int64_t tb3, int64_t db1, int64_t db2, int64_t db3, int64_t n_table_rows) {
    const int64_t r   = blockIdx.x;
    const int64_t i10 = r % ne10, i11 = (r / ne10) % ne11, i12 = r / (ne10 * ne11);
    int64_t row       = *(const int32_t*)(ids + i10 * ib0 + i11 * ib1 + i12 * ib2);
    row               = row < 0 ? 0 : (row >= n_table_rows ? n_table_rows - 1 : row);  // never read outside the table
    const char* src   = table + row * tb1 + i11 * tb2 + i12 * tb3;
    float* out        = (float*)((char*)dst + i10 * db1 + i11 * db2 + i12 * db3);
    for (int64_t c = threadIdx.x; c < nc; c += blockDim.x) {
        float v;
        if (TYPE == 0) {
            v = ((const float*)src)[c];
        } else if (TYPE == 1) {
            v = (float)((const _Float16*)src)[c];
        } else if (TYPE == 30) {
            v = __uint_as_float((uint32_t)((const uint16_t*)src)[c] << 16);
        } else if (TYPE == 8) {
            const char* blk = src + (c >> 5) * 34;
            v               = (float)*(const _Float16*)blk * (float)((const int8_t*)(blk + 2))[c & 31];
        } else {
            const char* blk = src + (c >> 5) * 18;
            const int j     = (int)(c & 31);
            const uint8_t q = ((const uint8_t*)(blk + 2))[j & 15];
            v               = (float)*(const _Float16*)blk * (float)((j < 16 ? (q & 0xF) : (q >> 4)) - 8);
        }
        out[c] = v;
    }
}
void launch_get_rows(hipStream_t s, float* dst, const int64_t dnb[4], const View4& table, const View4& ids) {
    const int64_t nr = ids.ne[0] * ids.ne[1] * ids.ne[2];
    if (nr == 0) return;
    const int threads = table.ne[0] >= 256 ? 256 : 64;
#define GR(T)                                                                                                                                                  \
    k_get_rows<T><<<(unsigned)nr, threads, 0, s>>>(dst, (const char*)table.data, (const char*)ids.data, table.ne[0], ids.ne[0], ids.ne[1], ids.nb[0], ids.nb[1], \
                                                  ids.nb[2], table.nb[1], table.nb[2], table.nb[3], dnb[1], dnb[2], dnb[3], table.ne[1])
    switch (table.type) {
        case 0: GR(0); break;
        case 1: GR(1); break;
        case 30: GR(30); break;
        case 8: GR(8); break;
        default: GR(2); break;
    }
#undef GR
}

}  // namespace mi355x
