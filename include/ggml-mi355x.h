/*
 * ggml-mi355x.h — C ABI exported by libggml-mi355x.so, the MI355X (gfx950) ggml backend plug-in.
 *
 * The library is a drop-in for the reference's ggml-backend compute path: a host that was built with
 * GGML_BACKEND_DL (the reference's CI does exactly this: .github/workflows/build.yml:88,686) discovers
 * it with ggml_backend_load_all(), enumerates its devices and drives it ONLY through the vtables of
 * include/ggml-abi.h.  Each entry point below cites the reference interface it plugs into.
 *
 *   ggml_backend_init()            <- dlsym'd by ggml_backend_load()/load_all()
 *                                     (src/core/ggml_extend_backend.cpp:302-320 -> ggml_backend_load_all)
 *   ggml_backend_score()           <- optional ranking among several libggml-*.so variants
 *   ggml_backend_mi355x_reg()      <- static-registration form (what ggml-backend-reg.cpp would call if
 *                                     the backend were compiled into ggml: `register_backend(ggml_backend_mi355x_reg())`)
 *
 * Reached through the returned registry (struct ggml_backend_reg, include/ggml-abi.h):
 *   reg.get_device(i)              <- ggml_backend_dev_get / dev_by_name (ggml_extend_backend.cpp:334-418)
 *   dev.supports_op(node)          <- probed at graph BUILD time (ggml_extend.hpp:1425, :2198-2210)
 *   dev.get_buffer_type / buft.alloc_buffer / buffer.set_tensor,get_tensor
 *                                  <- gallocr + weight staging (ggml_extend.hpp:2227-2245, 2347-2435;
 *                                     model_manager.cpp:470-477, 735-750)
 *   dev.init_backend -> backend.graph_compute(cgraph)
 *                                  <- THE hot-path call, src/core/ggml_extend_backend.cpp:471 (sync form)
 *                                     and :489 (async on a sub-graph VIEW: n_nodes slice, leafs == NULL)
 *   backend.synchronize            <- ggml_extend_backend.cpp:494,504; ggml_extend.hpp:1526,2330
 *   reg.get_proc_address(name)     <- "ggml_backend_split_buffer_type" / "ggml_backend_set_n_threads" /
 *                                     "ggml_backend_get_features" -> NULL (host handles absence,
 *                                     ggml_extend_backend.cpp:801-804,440-446,519-528);
 *                                     "ggml_backend_mi355x_get_stats" / "_set_option" -> the functions below
 *
 * Error behaviour (SURVEY.md §8(b) Errors): graph_compute returns GGML_STATUS_FAILED for an unsupported
 * node or a HIP launch error and GGML_STATUS_ALLOC_FAILED when an internal workspace cannot be
 * allocated — it never aborts; alloc_buffer returns NULL on hipMalloc failure.
 */
#ifndef GGML_MI355X_H
#define GGML_MI355X_H

#include "ggml-abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GGML_MI355X_API __attribute__((visibility("default")))

GGML_MI355X_API ggml_backend_reg_t ggml_backend_init(void);
GGML_MI355X_API int ggml_backend_score(void);
GGML_MI355X_API ggml_backend_reg_t ggml_backend_mi355x_reg(void);
GGML_MI355X_API int ggml_backend_mi355x_get_device_count(void);

/* execution statistics of the graph planner (process-wide, monotonically increasing) */
struct ggml_backend_mi355x_stats {
    int64_t graphs_computed;     /* graph_compute calls */
    int64_t plans_built;         /* plan-cache misses (topology seen for the first time) */
    int64_t nodes_seen;          /* ggml nodes in the graphs of plans built */
    int64_t kernels_planned;     /* kernel launches in plans built (after fusion) */
    int64_t kernels_launched;    /* kernel launches issued */
    int64_t fused_conv;          /* IM2COL+MUL_MAT+CONT(+ADD...) chains replaced by the implicit-GEMM conv */
    int64_t fused_conv_bounced;  /* ... of which had to bounce through scratch because dst aliased the input */
    int64_t fused_linear;        /* MUL_MAT(+bias)(+residual) on the MFMA weight GEMM */
    int64_t fused_norm;          /* GROUP_NORM/NORM + affine (+SiLU) */
    int64_t fused_geglu;
    int64_t fused_attention;     /* attention sub-graphs routed to the flash kernel */
    int64_t generic_matmul;      /* MUL_MAT on the generic exact-f32 path */
    int64_t swizzled_weight_bytes;
    int64_t graph_replays;       /* hipGraph replays (when graph capture is enabled) */
    int64_t fused_linear_geglu;  /* FF1 GEMM + GEGLU in one kernel (the [tokens][2*inner] tensor is never written) */
    int64_t split_k_gemms;       /* gemm16 contractions planned with a split-K workspace */
    int64_t head_major_gemms;    /* q/k/v projections that store the attention operand layout directly */
    int64_t fused_modulate;      /* LayerNorm + adaLN modulate written straight to the next GEMM's f16 operand image (DiT) */
    int64_t fused_gate;          /* Linear -> * gate -> + x folded into the GEMM epilogue (DiT) */
    int64_t fused_gelu;          /* fc1 -> GELU written as fc2's f16 operand image */
    int64_t fused_rope;          /* Rope::apply_rope node chains (cont/repeat/mul/add) replaced by one rotary kernel */
    int64_t fused_concat_heads;  /* token concat + head-major permute (+ f16 cast) of the MMDiT joint-attention operands in one pass */
    int64_t qgemv_linears;       /* q8_0 / q4_0 Linears planned on the in-register dequant kernel (raw blocks streamed, no f16 weight image) */
    int64_t fused_chan_add;      /* conv + ADD(time-embedding [1,1,C,N]) folded into the conv epilogue (ResBlock) */
    int64_t fused_proj_tokens;   /* SpatialTransformer 1x1 proj_in / proj_out run as token GEMMs (the NCHW <-> token transposes are not executed) */
    int64_t gemm_attention;      /* attention chains with head dims beyond the flash kernel (VAE d = 512) composed from MFMA GEMMs + f16 row softmax */
    int64_t fused_q16;           /* Q projections stored as the flash kernel's f16 head-major operand (the f32 CONT buffer is never written) */
    int64_t split_k_inlaunch;    /* split-K GEMMs whose slices are combined by the last-arriving workgroup of each output tile (no reduce pass) */
    int64_t qgemm16_linears;     /* q8_0 / q4_0 Linears with 3 .. qgemm16_max_rows activation rows on k_qgemm16: raw GGUF blocks streamed, dequantised in registers into MFMA fragments (no f16 weight image) */
    int64_t fgemv_linears;       /* f16 / f32 Linears with <= 16 activation rows on k_fgemv (one weight-streaming launch instead of SiLU + pack + GEMM + split-K reduce) */
    int64_t fused_presilu;       /* SiLU nodes in front of a few-row Linear applied by k_fgemv / k_qgemv while staging the rows (the UNARY node is not executed) */
    int64_t fused_sibling_linears; /* head-major projection GEMMs saved by running the q / k / v (or k / v) Linears of one attention as ONE launch over the shared operand */
    int64_t hoisted_kv_linears;  /* cross-attention K / V projections of the text context computed in grouped launches ahead of their graph position (results in the arena) */
    int64_t window_convs;        /* 3x3 convs planned on the LDS-window kernel (conv3w.hip) */
    int64_t hoisted_emb_linears; /* per-ResBlock SiLU(emb) -> Linear projections computed by one grouped weight-streaming launch ahead of their graph position */
    int64_t fused_rows16;        /* Linear (+bias, +residual) read only by a 1x1 conv (SpatialTransformer proj_out): written as the conv's f16 operand rows */
    int64_t fused_joint_qkv;     /* MMDiT streams whose fused qkv projection feeds the joint attention through k_joint_heads (no split copy, no separate norms / concats) */
    int64_t jit_images;          /* quantised Linears planned with a just-in-time f16 image (option jit_qimages: no cached image, rebuilt in front of every launch) */
    int64_t fused_cat_rows16;    /* CONCAT along the feature dimension read only by Linears: their f16 operand image assembled directly (FLUX single block) */
    int64_t fused_gn_stats;      /* split-K convs whose slab reduce also writes the statistics of the GroupNorm that reads the result (k_splitk_reduce_gn) */
    int64_t fused_ln_reduce;     /* split-K Linears whose slab reduce also writes the f16 operand image of the LayerNorm that reads the result (k_splitk_reduce_ln) */
    int64_t redirect_fallbacks;  /* graphs planned a second time without the joint-qkv pre-passes because a redirected projection was not taken by its Linear */
    int64_t fused_concat_gn;     /* skip-connection CONCATs never materialised: GroupNorm statistics / apply (and the skip conv's operand cast) read the two sources (plan_concat_gn) */
    int64_t fused_conv_scale;    /* Conv2d scales (SCALE s -> conv -> SCALE 1/s, the reference's SDXL VAE setting) folded into the operand image and the epilogue */
    int64_t view_graphs;         /* plans built for SUB-GRAPH VIEWS (sd_ggml_graph_view, src/core/ggml_extend_backend.cpp:449-463: leafs NULL / size 0) */
    int64_t plans_evicted;       /* cached plans (with their captured hipGraph) dropped by the LRU bound of the plan cache (option plan_cache_cap, default 512) */
    int64_t hoisted_mod_linears; /* DiT modulation Linears (FLUX Modulation / SD3 adaLN: one or two rows, raw q8_0 / q4_0 weights, same input vector) computed by ONE grouped weight-streaming launch ahead of their graph position */
    int64_t view_external_nodes; /* nodes of those slices treated as read outside the slice (parent use_counts > readers inside, the slice's last node and its sources) */
    int64_t qinloop_linears;     /* q8_0 / q4_0 Linears above k_qgemm16's row range planned on the pipelined 256 x 256 tile with the raw GGUF blocks dequantised INSIDE the main loop (k_gemm16<..., QT>): no f16 weight image, resident or rebuilt */
    int64_t flash_out_alias;     /* FLASH_ATTN_EXT -> VIEW -> CONT chains NOT written by the flash kernel itself because the graph allocator gave the CONT the block of a Q / K / V operand (the node runs plain, the CONT as a copy) */
    int64_t flash_slice_images;  /* token-slice views of an attention output registered on the flash kernel's f16 operand image (their Linears read runs of rows out of it: no f32 tensor, no pack pass) */
    int64_t flash_short_launches;   /* launch_flash_attn calls that took k_flash_short (65 .. 96 keys held in registers, one-pass softmax) */
    int64_t flash_qb2_launches;     /* ... that took the two-query-block max-slot kernel k_flash_attn<48, 2, FAST, MSLOT, QB = 2, NSEL> */
    int64_t flash_mslot_launches;   /* ... that took the one-block max-slot kernel (d = 40, f16 K / V) */
    int64_t flash_generic_launches; /* ... that took a !FAST instantiation (generic staging: f32 or strided K / V, d % 8 != 0) */
    int64_t fused_gn_epilogue;   /* GroupNorms (direct, or over a skip CONCAT) whose statistics pass was replaced by k_gn_finalize over the per-channel records the producing conv epilogues wrote (option fuse_gn_epilogue) */
    int64_t fused_tile_merge;    /* overlap merges of a VAE tile batch (MUL by the row ramps -> MUL by the column ramps -> per tile ADD in place / CPY into a view of the canvas) run as ONE gather launch of k_tile_merge (option fuse_tile_merge) */
    /* elementwise.hip: launches per kernel route, counted where each launcher chooses (per launch call, not per plan; a hipGraph replay launches without choosing) */
    int64_t ew_bin_same;         /* launch_binary: k_bin_same (same shape, contiguous, 16-byte aligned) */
    int64_t ew_bin_rowvec;       /* ... k_bin_rowvec ([ne0] over rows) */
    int64_t ew_bin_tokvec;       /* ... k_bin_tokvec ([C,1,N] over [C,L,N]) */
    int64_t ew_bin_chan;         /* ... k_bin_chan ([1,1,C,N'] over [W,H,C,N]) */
    int64_t ew_bin_generic;      /* ... k_bin_generic (byte strides, broadcast by modulo) */
    int64_t ew_copy_contig;      /* launch_copy: k_copy_contig */
    int64_t ew_copy_transpose;   /* ... k_transpose (LDS-tiled batched 2-D transpose) */
    int64_t ew_copy_rows;        /* ... k_copy_rows (rows of ne0 contiguous on both sides) */
    int64_t ew_copy_generic;     /* ... k_copy_generic */
    int64_t ew_concat_dim2;      /* launch_concat: k_concat_dim2 */
    int64_t ew_concat_planes;    /* ... k_concat_planes */
    int64_t ew_concat_generic;   /* ... k_concat */
    int64_t ew_tile_merge_v4;    /* launch_tile_merge: k_tile_merge<4> */
    int64_t ew_tile_merge_v1;    /* ... k_tile_merge<1> */
    /* conv3w.hip / gemm16.hip: conv launches per kernel route, counted where each launcher chooses (per launch call, as the ew_* fields are) */
    int64_t c3w_tw16_bn256;      /* launch_conv3w: k_conv3w<TW = 16, BN = 256> (16-wide maps, 256-column tile) */
    int64_t c3w_tw16_bn320;      /* ... k_conv3w<16, 320> */
    int64_t c3w_tw32_bn256;      /* ... k_conv3w<32, 256> */
    int64_t c3w_tw32_bn320;      /* ... k_conv3w<32, 320> */
    int64_t c3w_tw64_bn256;      /* ... k_conv3w<64, 256> */
    int64_t c3w_tw64_bn320;      /* ... k_conv3w<64, 320> */
    int64_t c3w_tw128_bn256;     /* ... k_conv3w<128, 256> */
    int64_t c3w_tw128_bn320;     /* ... k_conv3w<128, 320> */
    int64_t g16_conv_t128;       /* launch_gemm16_conv: k_gemm16<128, 128, CONV> */
    int64_t g16_conv_t128n64;    /* ... k_gemm16<128, 64, CONV> (the 64-column form: OC <= 64) */
    int64_t g16_conv_t256;       /* ... 256 x 128, eight waves */
    int64_t g16_conv_t256w;      /* ... 256 x 128, four waves */
    int64_t g16_conv_t160;       /* ... 256 x 160, four waves */
    int64_t g16_conv_t160n;      /* ... 256 x 160, eight waves */
    int64_t g16_conv_t320;       /* ... 256 x 320, pipelined */
    int64_t g16_conv_t256p;      /* ... 256 x 256, pipelined */
    int64_t g16_conv_splitk_reduce; /* plain k_splitk_reduce launches behind a split conv (either kernel family; not k_splitk_reduce_gn, not the in-launch combine) */
    int64_t g16_conv_wmajor;     /* conv launches (either kernel family) that took the weight-major workgroup order (option conv_wmajor) */
    /* guidance.hip: the device-resident sampler's glue around an inpaint / pix2pix UNet */
    int64_t fused_model_input;   /* [MUL by the step's c_in ->] [RESHAPE -> REPEAT over the K branches -> RESHAPE ->] CONCAT(dim 2) with the [REPEATed] concat latent run as ONE launch of k_model_input (option fuse_model_input) */
    int64_t fused_guidance3;     /* the six nodes of the three-conditioning CFG combine over views of one [per, 3, nb] tensor run as ONE launch of k_guidance3 (option fuse_guidance3) */
    int64_t ew_model_input_v4;   /* launch_model_input: k_model_input<4> (plane a multiple of 4 floats, bases 16-byte aligned); per launch call, as the ew_* fields above */
    int64_t ew_model_input_v1;   /* ... k_model_input<1> */
    /* gemm16.hip / qgemm.hip: Linear (weight MUL_MAT) launches per kernel route, counted where each launcher chooses (per launch call, as the g16_conv_* fields are) */
    int64_t lin_t128;            /* launch_gemm16_linear / _multi / _geglu: k_gemm16<128, 128> */
    int64_t lin_t128n64;         /* ... k_gemm16<128, 64> (narrow outputs, small grids, every in-launch K combine of such a shape) */
    int64_t lin_t256;            /* ... 256 x 128, eight waves */
    int64_t lin_t256w;           /* ... 256 x 128, four waves (option gemm16_tile only) */
    int64_t lin_t160;            /* ... 256 x 160, four waves */
    int64_t lin_t160n;           /* ... 256 x 160, eight waves */
    int64_t lin_t320;            /* ... 256 x 320, pipelined */
    int64_t lin_t256p;           /* ... 256 x 256, pipelined (f16 weight image) */
    int64_t lin_t192p;           /* ... 256 x 192, pipelined (f16 weight image) */
    int64_t lin_t256p_q8;        /* ... 256 x 256, raw q8_0 rows dequantised in the main loop */
    int64_t lin_t256p_q4;        /* ... 256 x 256, raw q4_0 rows */
    int64_t lin_t192p_q8;        /* ... 256 x 192, raw q8_0 rows */
    int64_t lin_t192p_q4;        /* ... 256 x 192, raw q4_0 rows */
    int64_t lin_streamk;         /* ... the stream-K instantiation of the 256 x 256 tile (option streamk) */
    int64_t lin_rowsplit_main;   /* ... the whole-rounds launch of a row split (option tail_split); its tail counts under the tile it takes */
    int64_t lin_multi;           /* launch_gemm16_linear_multi calls (the launch's tile is counted too) */
    int64_t lin_splitk_reduce;   /* k_splitk_reduce behind a slab-split Linear */
    int64_t lin_splitk_reduce_ln; /* k_splitk_reduce_ln behind one (fused_ln_reduce) */
    int64_t lin_geglu_pair;      /* launch_gemm16_linear_geglu on the 128-column value / gate pairing (the launch's tile is counted too) */
    int64_t lin_geglu16;         /* ... on the 16-column interleave */
    int64_t lin_qgemv;           /* launch_qgemv: k_qgemv (one or two activation rows) */
    int64_t lin_qgemv_rows4;     /* ... k_qgemv_rows<QT, 4> (3 .. 4 rows) */
    int64_t lin_qgemv_rows8;     /* ... k_qgemv_rows<QT, 8> (5 .. 8 rows, option qgemv_max_rows) */
    int64_t lin_qgemv_rows16;    /* ... k_qgemv_rows<QT, 16> (9 .. 16 rows) */
    int64_t lin_qgemv_group;     /* launch_qgemv_group */
    int64_t lin_qgemm16_rb1;     /* launch_qgemm16: k_qgemm16<QT, 1> (32-row tiles) */
    int64_t lin_qgemm16_rb2;     /* ... k_qgemm16<QT, 2> */
    int64_t lin_qgemm16_rb4;     /* ... k_qgemm16<QT, 4> */
    int64_t lin_qgemm16_reduce;  /* the slab reduce behind a split launch_qgemm16 */
    int64_t lin_fgemv_f16;       /* launch_fgemv: k_fgemv<f16 weights> */
    int64_t lin_fgemv_f32;       /* ... k_fgemv<f32 weights> */
    int64_t lin_wswz_q;          /* launch_wswz_q: just-in-time f16 weight image (option jit_qimages) */
    /* IP-Adapter cross-attention (option fuse_ip_attn) */
    int64_t fused_ip_attn;           /* attn2 pairs FLASH_ATTN_EXT(q,k,v) / FLASH_ATTN_EXT(q,k_ip,v_ip) -> SCALE -> ADD planned as ONE launch of k_flash_short_ip (per plan; a pair refused for the placement of its operands counts in flash_out_alias) */
    int64_t flash_short_ip_launches; /* launch_flash_attn_ip calls (per launch call, as flash_short_launches) */
    /* CLIP vision tower (option fuse_patch_embed) */
    int64_t fused_patch_embed;       /* CLIPVisionEmbeddings chains (REPEAT class, IM2COL .. CONT of the stride = kernel conv, CONCAT, ADD position) planned as ONE launch of k_patch_embed (per plan) */
    int64_t patch_embed_launches;    /* launch_patch_embed calls (per launch call) */
};
GGML_MI355X_API void ggml_backend_mi355x_get_stats(struct ggml_backend_mi355x_stats* out);
/* Host enum numbering, resolved BY NAME.  The numeric values of `enum ggml_op` / `enum ggml_unary_op` in ggml-abi.h are a recollection of upstream, and
 * the reference links a fork that adds ops (src/core/ggml_extend.hpp:1059,1088,3492): ggml_backend_init() looks up the host's ggml_op_name /
 * ggml_unary_op_name / ggml_type_name (dlsym over the loaded objects) and rebuilds the planner's op tables from the names; type numbers (part of the
 * GGUF file format) are verified.  A host that lacks a needed name, names two numbers alike, or numbers a type differently gets ZERO devices and the
 * reason on stderr and in ggml_backend_mi355x_enum_status().  A host that hides those functions can call ggml_backend_mi355x_resolve_enums() itself
 * BEFORE ggml_backend_init(); returns 0, or -1 with the tables unchanged.  get_enum_maps: host number -> ggml-abi.h number (GGML_OP_COUNT /
 * GGML_UNARY_OP_COUNT = unknown to this backend), 256 entries each. */
GGML_MI355X_API int ggml_backend_mi355x_resolve_enums(const char* (*op_name)(int), const char* (*unary_op_name)(int), const char* (*type_name)(int));
GGML_MI355X_API const char* ggml_backend_mi355x_enum_status(void);
GGML_MI355X_API void ggml_backend_mi355x_get_enum_maps(uint8_t* ops256, uint8_t* unary256);
/* live per-kernel-family timing (bench.py's roofline legs): while a family's bit is enabled, every dispatch of that family is bracketed by
 * HIP events recorded on the launch stream.  get_* synchronise the device, return the totals since enable / the last get_, and reset.
 * Family indices (bit positions of `family_mask`): 0 conv 256-row tiles, 1 conv 128-row tiles, 2 Linear GEMM, 3 flash attention,
 * 4 q8_0/q4_0 in-register dequant GEMM, 5 f32 MFMA matmul, 6 k_nchw_to_nhwc_f16, 7 k_layer_norm_f16, 8 k_gn_stats, 9 f16 pack,
 * 10 copies / transposes, 11 binary elementwise, 12 concat, 13 unary / scale, 14 split-K reduce, 15 f32 norms, 16 softmax, 17 other. */
struct ggml_backend_mi355x_kernel_timing {
    char kernel[96];     /* kernel family the events bracket */
    int64_t launches;
    double total_ms;     /* sum of hipEventElapsedTime over the launches */
    double total_flops;  /* sum of the launches' algorithmic FLOPs (conv: 2 * positions * IC*KH*KW * OC; attention: 4 * Lq * Lk * heads * d) */
    double total_bytes;  /* sum of the launches' algorithmic HBM bytes (bandwidth-bound families: one read + one write of the activation) */
    int32_t bound;       /* 0 = judged against the MFMA peak, 1 = against HBM bandwidth */
    int32_t family;
};
GGML_MI355X_API void ggml_backend_mi355x_kernel_timing_enable(int enable);           /* != 0: family 0 only (the dominant kernel; cheap enough for the timed region) */
GGML_MI355X_API void ggml_backend_mi355x_kernel_timing_enable_mask(uint32_t family_mask);
GGML_MI355X_API void ggml_backend_mi355x_get_kernel_timing(struct ggml_backend_mi355x_kernel_timing* out);  /* the first timed family */
GGML_MI355X_API int ggml_backend_mi355x_get_kernel_timings(struct ggml_backend_mi355x_kernel_timing* out, int capacity);  /* every family with launches; returns the count */
/* options (default): "fusion" (1), "mfma_gemm" (1), "hip_graph" (1: a plan is captured into a hipGraph the second time it runs and replayed from then on; 2 = capture at the first run; eager while kernel timing is on), "flash_pattern" (1), "gemm16_variant" (3), "gemm16_tile" (-1),
 * "splitk_target" (384), "conv_tap_major" (0), "fuse_modulate" / "fuse_gate" / "fuse_gelu" / "fuse_rope" / "fuse_concat_heads" (1);
 * "splitk_mid" (0: two K slices for launches of 193..384 workgroups), "pinned_uploads" (0: set_tensor_async stages through pinned host memory so the call does
 * not wait for the stream);
 * few-row / quantised Linears: "fgemv" (1: f16 / f32 weights under <= 16 rows on the one-launch weight-streaming kernel, SiLU in front of it applied on
 * load), "fgemv_max_rows" (16), "qgemv" (1) / "qgemv_max_rows" (4, <= 16: raw q8_0 / q4_0 blocks streamed up to that many rows), "qgemm16_max_rows" (512:
 * raw-block MFMA GEMM up to n rows; 8192 = the resident-quantised mode, no f16 image for any quantised Linear), "qgemm16" (1);
 * "fuse_linear_nchw" (1: Linear proj_out -> PERMUTE -> CONT -> RESHAPE -> ADD x_in of such a SpatialTransformer runs as a 1x1 implicit-GEMM conv over the token rows: NCHW + bias + residual epilogue),
 * "fuse_gn_tokens" (1: GroupNorm -> PERMUTE -> CONT -> Linear proj_in of a SpatialTransformer with Linear projections (SDXL): the GroupNorm apply pass writes the Linear's f16 operand image),
 * "fuse_concat_gn" (1: UNet skip-connection CONCAT read only by a GroupNorm chain (+ the skip 1x1 conv) is never built, option 0 = the concat pass),
 * "fuse_split_gelu" (1: FLUX linear1 writes gelu(mlp) as f16 into linear2's operand image), "geglu16" (1: GEGLU FF1 on the 256 x 320 tile through the 16-column
 * value / gate interleave), "streamk" (0; 1 / 2 / 3: stream-K policies for the pipelined 256 x 256 Linear tile), "qgemm16_rb" (3), "conv3w_prio" (3);
 * "relax_res_overlap" (1: a Linear + residual ADD fuses even when the allocator put the sum on the Linear input's released f32 buffer — GEMM launches read the
 * arena's f16 operand image, not that buffer; 0 = the round-3 test);
 * launch grouping: "fuse_siblings" (1: q / k / v projections of one attention as one multi-weight launch), "hoist_kv" (1: cross-attention K / V
 * projections of all blocks grouped ahead of their graph position, results in the arena); "fuse_q16", "fuse_chan_add", "fuse_proj_tokens" (1);
 * "hoist_emb" (1: the per-ResBlock SiLU(emb) -> Linear projections as one grouped weight-streaming launch), "fuse_joint_qkv" (1: MMDiT joint attention — qkv projections into arena scratch, split / per-head RMSNorm / token
 * concat / head-major cast as one pass per operand), "fuse_cat_rows16" (1: concat(a, b) along features feeding only Linears is assembled as their f16
 * operand image — flash output and gelu(strided view) write their columns themselves), "fuse_gn_stats" (1: the slab reduce of a split-K conv
 * also computes the statistics of the GroupNorm that reads its result), "fuse_rows16" (0: a Linear read only by a
 * 1x1 conv writes the conv's f16 operand rows; measured slightly slower on SD1.5);
 * "splitk_inkernel" (0: split-K combined by the last-arriving workgroup, 128-row tiles; measured slower) / "splitk_in_target" (320);
 * conv: "conv3w" (1: 3x3 / stride-1 convs on 16..128-wide maps on the LDS-window kernel), "conv3w_min_blocks" (8) / "conv3w_min_blocks_deep" (5:
 * least 32-channel blocks per K slice when the window kernel splits K);
 * round 5: "fuse_conv_scale" (1: Conv2d scale — SCALE s -> conv -> SCALE 1/s, the reference's SDXL VAE setting — folded into the operand image and the epilogue),
 * "conv_wmajor" (1: weight-major workgroup order for convs whose weight image is >= 2x their input image: every (column tile, K slice) weight chunk on one XCD),
 * "t256p_pad" (1: the pipelined 256 x 256 Linear tile also for widths that are multiples of 128 only), "tail_split" (0: row-split launches — whole rounds of 256 x 256
 * tiles + the remaining rows on small tiles; measured neutral), "ln16_rows" (1; 4 = four rows per wave in the LayerNorm -> f16 image kernel: measured slower);
 * round 6: "qinloop_min_rows" (513: q8_0 / q4_0 Linears with at least that many activation rows whose launch takes the pipelined 256 x 256 tile read the RAW GGUF blocks and
 * dequantise them inside the GEMM's main loop — no f16 weight image, cached or rebuilt; 0 = off: cached image, or "jit_qimages" rebuild),
 * "fuse_flash_slices" (1: the proj Linears of an MMDiT / FLUX double block read their token slices out of the flash kernel's f16 image), "gemm16_t192p" (1: the pipelined 256 x 192 Linear tile where it quantises better on 256 CUs), "hoist_mod" (1), "plan_cache_cap" (512), "gn_split_min" (65536);
 * "fuse_ip_attn" (1: the two attentions of an IP-Adapter attn2 — text keys and 1 .. 32 image keys of the same q — with their SCALE and ADD as one launch of
 * k_flash_short_ip; 0 = plain nodes on k_flash_short and the elementwise launches);
 * "fuse_patch_embed" (0 = plain nodes, the default: at batch 1 the one launch measured slower than they are, profiles/clip_vision_probe.txt; 1: the embeddings stage of a CLIP vision tower — REPEAT of the class embedding, the stride = kernel conv without bias (IM2COL .. CONT), the
 * transposing CONT, CONCAT and the ADD of the position table — as one launch of k_patch_embed);
 * "fuse_ln_reduce" (1: the slab reduce of a split-K Linear also writes the f16 operand image of the LayerNorm that reads its result);
 * "fuse_gn_epilogue" (1: an unsplit LDS-window conv read by a GroupNorm, or by a skip CONCAT a GroupNorm reads, writes per-channel (mean, M2) records of the values it
 * stores; the GroupNorm's statistics pass over the tensor becomes one small finalize launch over the records; 0 = the plan without it);
 * "fuse_tile_merge" (1: the overlap merge of a VAE tile batch — two MULs by the ramp vectors and one ADD in place / CPY per tile into views of the canvas — as one
 * launch of k_tile_merge: every canvas cell of the batch's bounding box is read and written once, results bit-identical to the plain nodes; timed in family 11);
 * "fuse_model_input" (1: the model input of the device-resident sampler on an inpaint / pix2pix UNet — x * c_in, tiled over the K branches of every image, with the
 * branch's constant concat latent appended along the channels — as one launch of k_model_input instead of MUL, REPEAT, [REPEAT,] CONCAT and three intermediates.
 * The MUL is folded in only when the chain is its sole reader; otherwise it runs and the kernel copies its result.  Refused — the nodes run plain — when an
 * intermediate is a graph output or has a reader outside the chain (a sub-graph view that cuts the chain included), when a tensor is not f32 or not contiguous;
 * bit-identical to the plain nodes; timed in family 12),
 * "fuse_guidance3" (1: the three-conditioning CFG combine iu + img * (u - iu) + txt * (c - u) over the views (c, u, iu) of one [per, 3, nb] tensor — SUB, MUL, ADD,
 * SUB, MUL, ADD — as one launch of k_guidance3, the two scales read from the step's scalar tensor on the device, every operation rounded on its own; the same
 * refusals; bit-identical to the plain nodes; timed in family 11).
 * An unknown key changes nothing and is named on stderr.  Wrong-result timing ablations exist only in builds with -DMI355X_EXPERIMENTS ("gemm16_abl"). */
GGML_MI355X_API void ggml_backend_mi355x_set_option(const char* key, int value);
/* What the calling thread's current device delivers, measured in about a second (csrc/kernels/calib.hip): an MFMA loop from registers (f16, 32x32x16: the
 * matrix pipe's ceiling at the clock the chip sustains under it, and that clock), a float4 copy and a read-only pass over 1 GiB.  bench.py reports them as
 * roofline.measured_peaks next to the vendor peaks, so that runs on boxes of different speed can be compared.  Returns 0, or -1 on failure. */
struct ggml_backend_mi355x_calibration {
    float mfma_f16_tflops; /* dense f16 MFMA, TFLOP/s */
    float mfma_clock_mhz;  /* shader clock during the MFMA loop */
    float copy_tbs;        /* (read + write bytes) / time of a float4 copy, TB/s */
    float read_tbs;        /* read-only pass, TB/s */
    int compute_units;
};
GGML_MI355X_API int ggml_backend_mi355x_calibrate(struct ggml_backend_mi355x_calibration* out);
/* the hipStream_t every graph of this backend instance is enqueued on (graph_compute_async, set/get_tensor_async): a caller that touches a
 * tensor's device memory between two graphs (the CFG-pair all-reduce, sd_set_pair_exchange) orders its work on this stream */
GGML_MI355X_API void* ggml_backend_mi355x_get_stream(ggml_backend_t backend);
/* The step caches' device passes (EasyCache / UCache on the device-resident sampler; kernels/step_cache.hip), enqueued on that stream between two graphs.  All
 * pointers are DEVICE addresses of f32 data; `stats` is 4 floats.  Both sums are deterministic (fixed grid, per-workgroup partials added in a fixed order by a second
 * one-workgroup launch, no floating-point atomics; at most 128 additions deep).  false: bad arguments or a size beyond that depth bound — nothing was enqueued.
 *   probe : stats[0] = sum over n of |x * c_in - prev_in|, the product rounded to f32 once (the step graph's MUL)
 *   record: in / prev_in / prev_out [per, nb], out / diff [per, k, nb] with k = 1 or 2 conditions adjacent per image, condition 0 first:
 *           diff_j = out_j - in, prev_in = in, prev_out = out_0, stats[1] = sum |out_0 - prev_out before this call| (0 and prev_out not read unless has_prev_out),
 *           stats[2] = sum |out_0| */
GGML_MI355X_API bool ggml_backend_mi355x_step_cache_probe(ggml_backend_t backend, const float* x, float c_in, const float* prev_in, int64_t n, float* stats);
GGML_MI355X_API bool ggml_backend_mi355x_step_cache_record(ggml_backend_t backend, const float* in, const float* out, float* prev_in, float* prev_out, float* diff, int64_t per,
                                                           int k, int64_t nb, bool has_prev_out, float* stats);
/*   probe_rel (the CacheDIT modes): stats[0] as probe, stats[3] = sum over n of |prev_in| — one pass and the finish launch, the same guarantees */
GGML_MI355X_API bool ggml_backend_mi355x_step_cache_probe_rel(ggml_backend_t backend, const float* x, float c_in, const float* prev_in, int64_t n, float* stats);
/* Spectrum's forecast (kernels/step_cache.hip), one streaming kernel on that stream: with H_j = ring + order[j] * slot_stride (k slots of n floats, oldest first,
 * 2 <= k <= 16) and every operation rounded to f32 on its own,
 *   pc = 0; for j: pc = pc + weights[j] * H_j[f];  pt = H_{k-1}[f] + 0.5 * (H_{k-1}[f] - H_{k-2}[f]);  out[f] = (1 - w) * pt + w * pc
 * order and weights are HOST arrays (passed as kernel arguments).  out must not overlap the ring.  false: bad arguments — nothing was enqueued. */
GGML_MI355X_API bool ggml_backend_mi355x_spectrum_predict(ggml_backend_t backend, const float* ring, int64_t slot_stride, const int* order, int k, const float* weights, float w,
                                                          int64_t n, float* out);
/* a computed step's `denoised` into its ring slot: a device-to-device copy of n floats enqueued on that stream (no kernel) */
GGML_MI355X_API bool ggml_backend_mi355x_spectrum_push(ggml_backend_t backend, const float* src, float* dst, int64_t n);
/* The latent previews' byte stages (kernels/preview.hip), enqueued on that stream between two graphs: the kernel writes a byte buffer the backend owns (made on first
 * use, grown on demand, freed with the backend) and ONE asynchronous device-to-host copy of plane * n * 3 bytes into out_rgb follows on the same stream — the caller
 * synchronises (ggml_backend_synchronize) before it reads them.  latents / chw: DEVICE addresses of planar f32 data; proj ([c][3]), bias ([3]) and out_rgb: HOST.
 *   latent_preview: [plane, c, n] -> RGB [n][plane][3].  v = x * in_scale (one rounded multiply, only when in_scale != 1); r = g = b = 0, for d ascending
 *                   r = r + v * proj[d][0] ... (multiply and add rounded separately); + bias; m * .5f + .5f; (0 < m) ? m : 0, (m < 1) ? m : 1 (NaN -> 0);
 *                   (uint8_t)(m * 255).  proj NULL (c must be 3): the channels are r, g, b and no bias is added; bias NULL: zeros.  c <= 128.
 *   planar_to_u8  : [plane, 3, n] -> RGB [n][plane][3].  v = x * in_mul + in_add (rounded separately, only when (in_mul, in_add) != (1, 0)); v <= 0 or NaN -> 0,
 *                   v >= 1 -> 255, else (uint8_t)(v * 255.0f + 0.5f).
 * false: bad arguments or no memory for the byte buffer — nothing was enqueued. */
GGML_MI355X_API bool ggml_backend_mi355x_latent_preview(ggml_backend_t backend, const float* latents, int64_t plane, int c, int64_t n, float in_scale, const float* proj,
                                                        const float* bias, uint8_t* out_rgb);
GGML_MI355X_API bool ggml_backend_mi355x_planar_to_u8(ggml_backend_t backend, const float* chw, int64_t plane, int64_t n, float in_mul, float in_add, uint8_t* out_rgb);
/* CLIP preprocessing (kernels/clip_vision.hip): n u8 HWC RGB pictures [n][h][w][3] -> pixel values [S, S, 3, n] f32 = (clamp(v / 255, 0, 1) - mean[c]) / std[c] of the
 * pixel (xi[x], yi[y]) — xi / yi: the S source columns / rows of the resize + centre crop (0 <= xi < w, 0 <= yi < h, checked).  images, xi, yi and out are HOST memory;
 * complete on return.  false: bad arguments or no memory */
GGML_MI355X_API bool ggml_backend_mi355x_clip_preprocess(ggml_backend_t backend, const uint8_t* images, int w, int h, int64_t n, int S, const int* xi, const int* yi, float* out);
/* path of the HIP runtime library this plug-in is bound to, and hipSetDevice through it (for companions that must share its streams: RCCL) */
GGML_MI355X_API const char* ggml_backend_mi355x_hip_library(void);
GGML_MI355X_API int ggml_backend_mi355x_set_device(int hip_device);
GGML_MI355X_API int ggml_backend_mi355x_get_device(void); /* the calling thread's current HIP device of the plug-in's runtime, -1 on error */

#ifdef __cplusplus
}
#endif
#endif
