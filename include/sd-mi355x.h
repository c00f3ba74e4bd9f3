/*
 * sd-mi355x.h — C ABI of the MI355X denoise + VAE-decode engine (libsdcpp-host.so).
 *
 * This is the host-facing slice of the reference's public C API (include/stable-diffusion.h) that the
 * hot path touches, with the same names / argument meaning / error behaviour where a counterpart
 * exists, and plain pointers + sizes everywhere (no C++ / torch types).  What differs, and why:
 *   - conditioning enters the denoise path as tensors (`sd_condition_t`, the SDCondition struct of
 *     src/conditioning/conditioner.hpp:18-34); the text encoders that produce them take token ids
 *     (sd_get_learned_condition below) because the reference's tokenizer vocabularies are not in its source drop;
 *   - weights are synthetic (random-init of the named architecture) unless the caller overwrites
 *     tensors by name with sd_set_tensor (checkpoint readers are a "next" row).
 *
 * All compute goes through ggml's backend plug-in interface (include/ggml-abi.h).  The engine loads
 * libggml-mi355x.so and FAILS (returns NULL) if it or a gfx950 device is missing — there is no CPU
 * fallback in the product.  Tests may register another backend plug-in (the CPU oracle) explicitly
 * through sd_load_backend() and select it by name.
 *
 * NAMING.  The reference's public API takes model paths and prompt strings and its parameter structs carry ~50 fields the hot path never
 * reads (include/stable-diffusion.h:192-287); this slice takes tensors and token ids, so its structs CANNOT be layout-compatible.  Every
 * type, enumerator and function whose name exists in the reference header therefore carries the prefix `sdm_` / `SDM_` here: a program
 * may include both headers and link both libraries, and a reference-side caller can never bind one of these entry points by accident
 * (round-1 review: same names + different layouts = silent memory corruption).  The pairs:
 *
 * reference (stable-diffusion.h)                  -> this header
 *   sd_ctx_params_t                     :192-238 -> sdm_ctx_params_t (only the fields the hot path reads; + model family, weight seed)
 *   sd_sample_params_t                  :276-287 -> sdm_sample_params_t
 *   sd_img_gen_params_t                          -> sdm_img_gen_params_t (conditioning as tensors instead of prompt strings)
 *   sd_image_t                          :258-263 -> sdm_image_t (same four fields, same order)
 *   enum sample_method_t / scheduler_t  :38-83   -> sdm_sample_method_t / sdm_scheduler_t (same numeric values for the members kept)
 *   enum sd_type_t                      :99-143  -> sdm_type_t (same numeric values = enum ggml_type)
 *   new_sd_ctx / free_sd_ctx            :482-485 -> sdm_new_ctx / sdm_free_ctx
 *   generate_image                      :493-496 -> sdm_generate_image (batch_count images, seeds seed+b)
 *   free_sd_images                      :595-597 -> sdm_free_images
 *   sd_*_params_init                             -> sdm_*_params_init
 *   sd_set_backend_eval_callback        :442-447 -> sdm_set_backend_eval_callback (sub-graph views are honoured by the backend)
 *   sd_img_gen_params_t::init_image / mask_image / strength -> sdm_img_gen_params_t::init_latent (sd_vae_encode) / denoise_mask / strength
 *   sd_sample_params_t::custom_sigmas / flow_shift / guidance.slg -> the same fields of sdm_sample_params_t (slg_*)
 *   sd_ctx_params_t::prediction / taesd_path     -> sd_set_prediction / sd_use_tae + sd_load_weights_prefixed(ctx, file, "tae.")
 * Names without a reference counterpart (sd_unet_forward, sd_vae_decode, sd_load_backend, ...) keep the plain `sd_` prefix.
 */
#ifndef SD_MI355X_H
#define SD_MI355X_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_API __attribute__((visibility("default")))

enum sd_model_family_t {
    SD_MODEL_SD15       = 0, /* UNetConfig defaults, unet.hpp:16-35; VAE 4ch scale 0.18215 */
    SD_MODEL_SDXL       = 1, /* unet.hpp:47-57; VAE scale 0.13025 */
    SD_MODEL_SD15_TINY  = 2, /* same topology, model_channels 32 — CPU-sized parity tests */
    SD_MODEL_SDXL_TINY  = 3,
    SD_MODEL_SD35_LARGE = 4, /* MMDiT, 38 joint blocks, hidden 2432, rms qk-norm (mmdit.hpp); 16-ch VAE scale 1.5305 shift 0.0609;
                                discrete-flow denoiser, shift 3.0 (denoiser.hpp:1239-1283) */
    SD_MODEL_SD35_TINY  = 5, /* same topology at 3 blocks / hidden 192, with one MMDiT-X self-attention block */
    SD_MODEL_FLUX_DEV   = 6, /* FLUX.1-dev: 19 double + 38 single stream blocks, hidden 3072, 24 heads, RoPE axes 16/56/56, distilled
                                guidance input (flux.hpp); 16-ch VAE scale 0.3611 shift 0.1159; FluxFlowDenoiser + Flux scheduler */
    SD_MODEL_FLUX_TINY  = 7, /* same topology: 2 + 2 blocks, hidden 128, 4 heads, axes 8/12/12 */
    SD_MODEL_SD35_WIDE2 = 8, /* SD3.5-large's real width (hidden 2432, 38 heads x 64), 2 joint blocks — full-width block parity tests */
    SD_MODEL_FLUX_WIDE1 = 9, /* FLUX.1-dev's real width (hidden 3072, 24 heads x 128), 1 double + 1 single block — same purpose */
    SD_MODEL_SD3M_TINY  = 10, /* SD3-medium's topology at test size: MMDiT WITHOUT qk-norm and without MMDiT-X blocks (mmdit.hpp:299-366 with qk_norm = "") */
    SD_MODEL_SD35_WIDE8 = 11, /* SD3.5-large's real width, 8 joint blocks: the middle point of the depth sweep (2 / 8 / 38) of tests/test_zz_gpu_fulldepth.py */
    SD_MODEL_FLUX_WIDE8 = 12, /* FLUX.1-dev's real width, 3 double + 5 single blocks: the middle point of the FLUX depth sweep (1+1 / 3+5 / 19+38) */
};

/* numeric values = enum ggml_type (stable-diffusion.h:98-143) */
enum sdm_type_t {
    SDM_TYPE_F32  = 0,
    SDM_TYPE_F16  = 1,
    SDM_TYPE_Q4_0 = 2,
    SDM_TYPE_Q8_0 = 8,
    SDM_TYPE_BF16 = 30,
};

/* SDM_SAMPLE_METHOD_COUNT = "the family's default" like the reference's SAMPLE_METHOD_COUNT (sd_get_default_sample_method,
 * stable-diffusion.cpp:3965-3975): Euler for the DiT families (SD3.5, FLUX), Euler-A otherwise */
/* Numeric values = the reference's sample_method_t / scheduler_t (include/stable-diffusion.h:38-83), so integers a host already holds keep their meaning.  Implemented
 * (host-side math, bit-for-bit against src/runtime/denoiser.hpp compiled from the reference: tests/test_host_logic.py): EVERY method sample_k_diffusion dispatches, 0 ... 20 (the `extra_sample_args` knobs of LMS / Euler GE / LCM
 * at their defaults); schedulers DISCRETE, KARRAS, EXPONENTIAL, AYS, GITS, SGM_UNIFORM, SIMPLE, SMOOTHSTEP, KL_OPTIMAL, LCM, BONG_TANGENT, BETA (alpha = beta = 0.6) and FLUX — every
 * scheduler_t value but the default ladders of model families outside this engine (LTX2 = 11, LOGIT_NORMAL = 12, FLUX2 = 13).  Any other value makes sdm_generate_image / sdm_sample_latents fail with an error message
 * (sd_last_error) instead of silently sampling something else.  SDM_SCHEDULER_COUNT = "the default for this model and method" (sd_get_default_scheduler,
 * stable-diffusion.cpp:3977-3998): LCM for the LCM and TCD methods, SIMPLE for DDIM trailing, FLUX for FLUX, DISCRETE otherwise.  Euler / Euler-A (and DDIM trailing, which the
 * reference runs as Euler-A) take the device-resident sampler; the multi-stage and multi-step methods run the host loop around the device forward. */
enum sdm_sample_method_t {
    SDM_EULER_SAMPLE_METHOD = 0, SDM_EULER_A_SAMPLE_METHOD = 1, SDM_HEUN_SAMPLE_METHOD = 2, SDM_DPM2_SAMPLE_METHOD = 3, SDM_DPMPP2S_A_SAMPLE_METHOD = 4,
    SDM_DPMPP2M_SAMPLE_METHOD = 5, SDM_DPMPP2Mv2_SAMPLE_METHOD = 6, SDM_IPNDM_SAMPLE_METHOD = 7, SDM_IPNDM_V_SAMPLE_METHOD = 8, SDM_LCM_SAMPLE_METHOD = 9,
    SDM_DDIM_TRAILING_SAMPLE_METHOD = 10, SDM_TCD_SAMPLE_METHOD = 11, SDM_RES_MULTISTEP_SAMPLE_METHOD = 12, SDM_RES_2S_SAMPLE_METHOD = 13, SDM_ER_SDE_SAMPLE_METHOD = 14,
    SDM_EULER_CFG_PP_SAMPLE_METHOD = 15, SDM_EULER_A_CFG_PP_SAMPLE_METHOD = 16, SDM_EULER_GE_SAMPLE_METHOD = 17, SDM_DPMPP2M_SDE_SAMPLE_METHOD = 18,
    SDM_DPMPP2M_SDE_BT_SAMPLE_METHOD = 19, SDM_LMS_SAMPLE_METHOD = 20, SDM_SAMPLE_METHOD_COUNT = 21
};
enum sdm_scheduler_t {
    SDM_DISCRETE_SCHEDULER = 0, SDM_KARRAS_SCHEDULER = 1, SDM_EXPONENTIAL_SCHEDULER = 2, SDM_AYS_SCHEDULER = 3, SDM_GITS_SCHEDULER = 4, SDM_SGM_UNIFORM_SCHEDULER = 5,
    SDM_SIMPLE_SCHEDULER = 6, SDM_SMOOTHSTEP_SCHEDULER = 7, SDM_KL_OPTIMAL_SCHEDULER = 8, SDM_LCM_SCHEDULER = 9, SDM_BONG_TANGENT_SCHEDULER = 10, SDM_FLUX_SCHEDULER = 14,
    SDM_BETA_SCHEDULER = 15, SDM_SCHEDULER_COUNT = 16
};

/* prediction_t of the reference (include/stable-diffusion.h), the two UNet parameterisations: sd_set_prediction */
enum sdm_prediction_t { SDM_EPS_PRED = 0, SDM_V_PRED = 1 };

typedef struct {
    const char* backend;        /* ggml device name, case-insensitive; NULL -> "MI355X0" (stable-diffusion.h:232) */
    enum sd_model_family_t model;
    enum sdm_type_t wtype;       /* Linear weight type (conv stays f16, norms/bias f32 — SURVEY.md F9) */
    bool diffusion_flash_attn;  /* stable-diffusion.h:223 */
    bool diffusion_conv_direct; /* stable-diffusion.h:225 */
    bool vae_decode_only;       /* always true here */
    uint64_t weight_seed;       /* synthetic-weight seed (1234) */
    int n_threads;              /* only reaches CPU backends (ggml_extend.hpp:2838-2843) */
} sdm_ctx_params_t;

typedef struct {
    float txt_cfg;              /* cfg scale (7.0 default, stable-diffusion.cpp:3650-3667) */
    enum sdm_scheduler_t scheduler;
    enum sdm_sample_method_t sample_method;
    int sample_steps;
    float eta;                  /* INFINITY -> 1.0 for Euler-A (stable-diffusion.cpp:4024-4049) */
    const float* custom_sigmas; /* sd_sample_params_t::custom_sigmas: count > 1 replaces the scheduler's ladder as it is (last value normally 0) */
    int custom_sigmas_count;
    const int* slg_layers;      /* skip-layer guidance (sd_slg_params_t; SD3.x): joint blocks left out of one more conditional forward per step inside the window */
    int slg_layer_count;        /* (slg_layer_start, slg_layer_end) x the ladder length; guided += (cond - skip) * slg_scale (guidance.cpp:296-340).  scale 0 = off */
    float slg_layer_start, slg_layer_end, slg_scale;
    float apg_eta, apg_momentum, apg_norm_threshold, apg_norm_threshold_smoothing; /* adaptive projected guidance (the reference's extra_sample_args apg_eta / apg_momentum /
                                   apg_norm_threshold / apg_norm_threshold_smoothing; AdaptiveProjectedGuidance, guidance.cpp:209-294) in place of plain CFG on the
                                   (cond, uncond) pair; neutral values (1, 0, 0, 0) = off */
    int shifted_timestep;       /* sd_sample_params_t::shifted_timestep (timestep-shifted distilled UNets): > 0: the model sees round(t * shifted_timestep / 1000) and that
                                   timestep's output scalings (prepare_sample_timesteps / adjust_sample_step_scalings, stable-diffusion.cpp:2411-2457); 0 = off */
    float flow_shift;           /* flow families: the time shift of DiscreteFlowDenoiser (set_flow_shift, stable-diffusion.cpp:3106-3115); INFINITY = the default (SD3.x 3.0, FLUX.1-dev 1.15) */
} sdm_sample_params_t;

/* SDCondition (conditioner.hpp:18-34): c_crossattn [ctx_dim, n_tokens], c_vector [adm] (SDXL) */
typedef struct {
    const float* c_crossattn;
    int64_t ctx_dim, n_tokens;
    const float* c_vector; /* NULL for SD1.x */
    int64_t vector_dim;
} sd_condition_t;

typedef struct {
    sd_condition_t cond;
    sd_condition_t uncond;      /* used iff txt_cfg != 1 (stable-diffusion.cpp:4249) */
    int width, height;          /* pixels; latent = /8 */
    sdm_sample_params_t sample_params;
    int64_t seed;
    int batch_count;            /* images seed .. seed+batch_count-1 (stable-diffusion.cpp:5664-5683) */
    int device_batch;           /* OUR extension: images denoised together per graph; 0 -> batch_count */
    bool decode;                /* run the VAE and return pixels; false -> latents only */
    bool fuse_cfg_pair;         /* OUR extension: cond and uncond of every image run in ONE graph (N = 2*batch, context [.,.,2]
                                   tiled by the graph's own ggml_repeat, unet.hpp:548-552) instead of two computes per step */
    bool device_sampler;        /* OUR extension: the whole iteration — x*c_in, model pair, CFG combine, Euler(-A) update —
                                   is one graph per step on latents that stay in a backend buffer; nothing crosses back to the host until
                                   the last step (the reference's three crossings per model call: stable-diffusion.cpp:2636-2664, 2855-2896) */
    const float* init_latent;   /* img2img (stable-diffusion.h init_image, already encoded: sd_vae_encode): diffusion latents [w/8, h/8, C] shared by the batch like the
                                   reference's one init image; the trajectory starts from noise_scaling(sigma_0, noise, init_latent) (denoiser.hpp:1181-1186, 1274-1279);
                                   NULL = txt2img */
    const float* denoise_mask;  /* inpainting (stable-diffusion.h mask_image, at latent resolution): [w/8, h/8] f32, 1 = repaint, 0 = keep; with init_latent every denoised
                                   prediction becomes denoised * mask + init_latent * (1 - mask) (stable-diffusion.cpp:2888-2890); NULL = none */
    float strength;             /* with init_latent: < 1 keeps the last t_enc + 2 sigmas of the ladder, t_enc = (int)(steps * strength) (stable-diffusion.cpp:4940-4980); 0.75 default */
} sdm_img_gen_params_t;

typedef struct {
    uint32_t width, height, channel;
    uint8_t* data;
} sdm_image_t;

typedef struct sdm_ctx_t sdm_ctx_t;

/* ---- backend discovery (GGML_BACKEND_DL) ---- */
SD_API bool sd_load_backend(const char* path); /* dlopen a libggml-<name>.so and register its devices */
SD_API int sd_device_count(void);
SD_API const char* sd_device_name(int i);
SD_API const char* sd_device_description(int i);

/* ---- context ---- */
SD_API void sdm_ctx_params_init(sdm_ctx_params_t* p);
SD_API void sdm_sample_params_init(sdm_sample_params_t* p);
SD_API void sdm_img_gen_params_init(sdm_img_gen_params_t* p);
SD_API sdm_ctx_t* sdm_new_ctx(const sdm_ctx_params_t* params); /* NULL on failure (no device, alloc failure) */
SD_API void sdm_free_ctx(sdm_ctx_t* ctx);
SD_API const char* sd_last_error(void);
/* UNet variants whose first conv is wider than the latent: the SD1.x / SDXL inpainting checkpoints (9 input channels: x 4 | mask 1 | masked-image latent 4, the
 * concat order of stable-diffusion.cpp:5166-5169) and the instruct-pix2pix edit checkpoints (8: x 4 | image latent 4), the reference's VERSION_*_INPAINT /
 * VERSION_*_PIX2PIX (src/model_loader.cpp: input_blocks.0.0.weight ne[2] == 9 / 8).  Only "model.diffusion_model.input_blocks.0.0.weight" changes shape
 * ([3,3,9|8,mc]; synthetic weights from the same seeded initialiser, sd_load_weights takes a real one); out channels, the latent (noise, x, VAE) and everything else
 * stay the family's.  The extra channels enter every model call as c_concat (unet.hpp:554-559): sd_unet_forward_concat, sd_set_concat_condition.
 * Valid for SD_MODEL_SD15 / SDXL / SD15_TINY / SDXL_TINY; any other family with a non-plain variant returns NULL (sd_last_error).  sdm_new_ctx(p) is
 * sdm_new_ctx_variant(p, SDM_UNET_PLAIN).  (A separate entry point and not a field: sdm_ctx_params_t is mirrored by every binding.)
 * SD1.x pix2pix quirk of the reference: sd_vae_encode on an SD15 / SD15_TINY PIX2PIX context returns the MEAN of the moments, neither sampled nor scaled to the
 * diffusion range (auto_encoder_kl.hpp:764-765, stable-diffusion.cpp:3056-3058); SDXL pix2pix encodes normally. */
enum sdm_unet_variant_t { SDM_UNET_PLAIN = 0, SDM_UNET_INPAINT = 1, SDM_UNET_PIX2PIX = 2 };
SD_API sdm_ctx_t* sdm_new_ctx_variant(const sdm_ctx_params_t* params, int variant);
SD_API int sd_unet_variant(sdm_ctx_t* ctx);
SD_API int sd_concat_channels(sdm_ctx_t* ctx);   /* 0, 5 or 4 */
/* reads only the header of a safetensors / GGUF / PyTorch checkpoint, finds "model.diffusion_model.input_blocks.0.0.weight" after name conversion (a diffusers
 * "conv_in.weight" counts) and returns the variant from its input width ne[2]: 4 -> 0, 9 -> 1, 8 -> 2; -1 (sd_last_error) when the tensor is absent or has another width */
SD_API int sd_probe_unet_variant(const char* path);

/* ---- weights by name ("model.diffusion_model.<...>", "first_stage_model.<...>") ---- */
SD_API int64_t sd_tensor_count(sdm_ctx_t* ctx);
SD_API const char* sd_tensor_name(sdm_ctx_t* ctx, int64_t i);
/* ne[4], ggml type; returns false if unknown */
SD_API bool sd_tensor_info(sdm_ctx_t* ctx, const char* name, int64_t* ne, int* type, size_t* nbytes);
SD_API bool sd_get_tensor(sdm_ctx_t* ctx, const char* name, void* dst, size_t nbytes);       /* raw bytes (device -> host) */
SD_API bool sd_get_tensor_f32(sdm_ctx_t* ctx, const char* name, float* dst, int64_t nelem);  /* dequantised */
SD_API bool sd_set_tensor_f32(sdm_ctx_t* ctx, const char* name, const float* src, int64_t nelem); /* converts per stored type */

/* ---- checkpoint files, told apart by their first bytes:
 *   safetensors          F32 / F16 / BF16 native; F64 / I64 / F8_E4M3 / F8_E5M2 widened at load
 *   GGUF v2 / v3         F32 / F16 / BF16 / Q8_0 / Q4_0 native; Q4_1 / Q5_0 / Q5_1 / Q2_K / Q3_K / Q4_K / Q5_K / Q6_K / IQ4_NL decoded at load
 *   PyTorch checkpoints  torch.save's zip container (.ckpt / .pt / .pth / .bin, PyTorch >= 1.6) and the legacy stream: float / half / bfloat16 /
 *                        double / long storages of contiguous tensors, found in the root dictionary and the dictionaries nested in it ("state_dict");
 *                        the pickle is interpreted, never executed (csrc/host/torch_ckpt_io.hpp)
 * Every parameter the model declares that the file names (original-LDM / sd.cpp GGUF names, e.g. "model.diffusion_model.input_blocks.0.0.weight")
 * is converted file dtype -> f32 -> the parameter's type (ModelLoader convert_tensor, src/model_loader.cpp:155-205) and uploaded.
 * Returns the number of parameters loaded, -1 on error (sd_last_error); *n_missing = declared but absent, *n_unused = in the file but unknown. */
SD_API int64_t sd_load_weights(sdm_ctx_t* ctx, const char* path, int64_t* n_missing, int64_t* n_unused);
/* Same, with `prefix` prepended to every file name first — diffusers keeps one file per sub-model whose names carry no component prefix
 * ("unet." / "vae." / "text_encoder." / "text_encoder_2.", model_loader.cpp init_from_diffusers_file).  File names are rewritten to the
 * engine's canonical dialect before matching (src/name_conversion.cpp): diffusers UNet / VAE names, OpenCLIP text-tower names (fused
 * in_proj rows are split into q/k/v), "conditioner.embedders.N.", "te1." … component aliases, llama.cpp-style T5 GGUF names. */
SD_API int64_t sd_load_weights_prefixed(sdm_ctx_t* ctx, const char* path, const char* prefix, int64_t* n_missing, int64_t* n_unused);
SD_API bool sd_convert_tensor_name(sdm_ctx_t* ctx, const char* name, char* out, size_t out_capacity); /* convert_tensor_name, name_conversion.cpp:1346 */

/* ---- the hot path ---- */
/* one diffusion-model forward (DiffusionModelRunner::compute, unet.hpp:818-858): x [W,H,C,N] f32,
 * timesteps [N], context [ctx_dim,n_tokens,N or 1], y [adm,N or 1] or NULL -> out [W,H,C,N] */
SD_API bool sd_unet_forward(sdm_ctx_t* ctx, const float* x, int w, int h, int c, int n, const float* timesteps,
                            const float* context, int64_t ctx_dim, int64_t n_tokens, int64_t ctx_n,
                            const float* y, int64_t y_dim, int64_t y_n, float* out);
/* the forward of an inpaint / pix2pix UNet (sdm_new_ctx_variant): c_concat [w,h,cc,concat_n], concat_n 1 or n, cc = sd_concat_channels(ctx).  The graph emits what
 * UnetModelBlock::forward emits (unet.hpp:554-559): [REPEAT to batch n,] CONCAT(x, c_concat, dim 2) in front of input_blocks.0.0.  sd_unet_forward on a variant
 * context is an error ("model needs c_concat"), never a silent zero-fill; so is a wrong cc */
SD_API bool sd_unet_forward_concat(sdm_ctx_t* ctx, const float* x, int w, int h, int c, int n, const float* timesteps, const float* context, int64_t ctx_dim, int64_t n_tokens,
                                   int64_t ctx_n, const float* y, int64_t y_dim, int64_t y_n, const float* c_concat, int cc, int concat_n, float* out);
/* ---- IP-Adapter (src/model/adapter/ip_adapter.hpp, CrossAttention::to_k_ip / to_v_ip, block.hpp:307-393); UNet families only.
 * The plain adapters (ImageProjModel: Linear + LayerNorm) here; the Resampler of the "plus" adapters (sd_ip_adapter_init_plus; its feed-forward is GELU_ERF, which the
 * MI355X backend runs and the CPU oracle of the tests does not) and the CLIP vision tower that makes the embeddings from a picture (sd_clip_vision_init,
 * sd_set_ip_adapter_image) follow below.  A caller with embeddings or tokens from elsewhere passes them to sd_ip_adapter_project / sd_set_ip_adapter directly.
 * sd_ip_adapter_init adds "...attn2.to_k_ip.weight" / "...attn2.to_v_ip.weight" [ip_dim -> inner, no bias] to every attn2 and "ip_adapter.image_proj.{proj,norm}.*", in a
 * weight buffer of their own with synthetic values from the seeded initialiser (sd_set_tensor_f32 binds real ones); the resident weights stay untouched.  A second
 * call with the same dimensions is a no-op, with other dimensions an error. */
SD_API bool sd_ip_adapter_init(sdm_ctx_t* ctx, int64_t ip_dim, int64_t clip_dim, int64_t num_tokens, uint64_t weight_seed);
/* an adapter file (safetensors / the formats sd_load_weights reads): names converted by the reference's rule (name_conversion.cpp:1307-1344; "ip_adapter.<idx>.to_k_ip.weight" ->
 * "model.diffusion_model.<block>.attn2.to_k_ip.weight", "image_proj.*" -> "ip_adapter.image_proj.*"), the adapter initialised from the file's shapes if it is not yet, its
 * parameters (and only they) bound.  Returns the number loaded or -1; n_missing counts adapter parameters the file lacks, n_unused file tensors nothing took */
SD_API int64_t sd_load_ip_adapter(sdm_ctx_t* ctx, const char* path, int64_t* n_missing, int64_t* n_unused);
SD_API bool sd_ip_adapter_info(sdm_ctx_t* ctx, int64_t* ip_dim, int64_t* clip_dim, int64_t* num_tokens); /* false: no adapter initialised */
/* ImageProjModel: CLIP image embeddings [clip_dim, n] -> image tokens tokens_out [ip_dim, num_tokens, n].  On a plus adapter: the tower's hidden states
 * [embed_dim, n_tok, n] with n_tok the token count of the context's vision tower (257 for 224 / 14); without a tower use sd_ip_adapter_project_tokens */
SD_API bool sd_ip_adapter_project(sdm_ctx_t* ctx, const float* embeds, int n, float* tokens_out);
/* the same with the token count stated: embeds [clip_dim, n_tok, n]; n_tok must be 1 on a plain adapter.  A backend without GELU_ERF refuses a plus adapter here */
SD_API bool sd_ip_adapter_project_tokens(sdm_ctx_t* ctx, const float* embeds, int64_t n_tok, int n, float* tokens_out);
/* The "plus" adapters: to_k_ip / to_v_ip as sd_ip_adapter_init plus the Resampler (ip_adapter.hpp:34-113) "ip_adapter.image_proj.{latents, proj_in, proj_out, norm_out,
 * layers.<i>.0.{norm1,norm2,to_q,to_kv,to_out}, layers.<i>.1.{0,1,3}}": `depth` layers of a cross-attention of num_queries latents [dim] onto the hidden states
 * [embed_dim] and a GELU_ERF feed-forward [ff_inner]; heads = dim / 64; output [ip_dim, num_queries].  A context holds ONE adapter, plain or plus.
 * sd_load_ip_adapter tells a plus file by "image_proj.latents" and reads the shapes as IPAdapterRunner does (ip_adapter.hpp:128-158) */
SD_API bool sd_ip_adapter_init_plus(sdm_ctx_t* ctx, int64_t ip_dim, int64_t dim, int64_t depth, int64_t num_queries, int64_t embed_dim, int64_t ff_inner, uint64_t weight_seed);
/* sd_ip_adapter_info plus is_plus (clip_dim is then the Resampler's embed_dim, num_tokens its num_queries) */
SD_API bool sd_ip_adapter_info_ex(sdm_ctx_t* ctx, int64_t* ip_dim, int64_t* clip_dim, int64_t* num_tokens, bool* is_plus);
/* ---- CLIP vision tower (src/model/te/clip.hpp:183-238, 332-464: CLIPVisionModelProjection) — what makes the image embeddings from a picture.
 * version 0 / 1 / 2 = ViT-L/14, ViT-H/14, ViT-bigG/14 (the reference's hyper-parameters; its MLP activation is tanh-GELU for hidden 1024 / 1280 and quick-GELU
 * otherwise, so also for bigG's 1664); `tiny` non-NULL overrides it with a test-width configuration (intermediate = 2 hidden).  Parameters "clip_vision.vision_model.*",
 * "clip_vision.visual_projection.weight" (f16 patch weight, f32 class embedding and position table) in a weight buffer of their own, synthetic values from the seeded
 * initialiser.  A second call with the same shape is a no-op, with another shape an error. */
typedef struct {
    int64_t hidden_size, n_head, n_layer, image_size, patch_size, projection_dim;
} sd_clip_vision_tiny_t;
typedef struct {
    int64_t image_size, patch_size, hidden_size, intermediate_size, n_head, n_layer, projection_dim, num_positions, use_gelu;
} sd_clip_vision_info_t;
SD_API bool sd_clip_vision_init(sdm_ctx_t* ctx, int version, const sd_clip_vision_tiny_t* tiny, uint64_t weight_seed);
SD_API bool sd_clip_vision_info(sdm_ctx_t* ctx, sd_clip_vision_info_t* out); /* false: no tower initialised */
/* a tower file (HF CLIPVisionModelWithProjection names), loaded under the "clip_vision." prefix by the reference's name rule (name_conversion.cpp:1473, :106-185); the
 * tower is initialised from the file's shapes if it is not yet.  Returns the number loaded or -1; n_missing / n_unused as sd_load_ip_adapter */
SD_API int64_t sd_load_clip_vision(sdm_ctx_t* ctx, const char* path, int64_t* n_missing, int64_t* n_unused);
/* clip_preprocess (src/core/util.cpp:695-758) of n u8 HWC RGB pictures [n][h][w][3]: value / 255, nearest resize by the larger of the two ratios (resized extents
 * truncated), centre crop, clamp to [0, 1], (v - mean) / std -> out [S, S, 3, n] with S the tower's image size (sd_clip_preprocess_size: S given, no tower needed).
 * One kernel launch on the MI355X backend; bit-equal to a NumPy restatement */
SD_API bool sd_clip_preprocess(sdm_ctx_t* ctx, const uint8_t* images, int w, int h, int n, float* out);
SD_API bool sd_clip_preprocess_size(sdm_ctx_t* ctx, const uint8_t* images, int w, int h, int n, int size, float* out);
/* pixel_values [S, S, 3, n] -> return_pooled: visual_projection(post_layernorm(x)[token 0]) [projection_dim, n]; else the hidden state BEFORE post_layernorm
 * [hidden, num_positions, n] (clip.hpp:389).  clip_skip > 0 stops n_layer - clip_skip + 1 layers in, pooled or not (clip.hpp:377) */
SD_API bool sd_clip_vision_encode(sdm_ctx_t* ctx, const float* pixel_values, int n, bool return_pooled, int clip_skip, float* out);
/* compute_ip_adapter_tokens (stable-diffusion.cpp:2187-2215) of one u8 HWC RGB picture: preprocess, encode (pooled for a plain adapter, the hidden state at clip_skip 2
 * for a plus one), project; uncond tokens from an all-zero embedding of the same shape; then sd_set_ip_adapter.  NULL clears.  An error (never a no-op) without a
 * tower, without an adapter, or when the tower's output width is not what the adapter expects */
SD_API bool sd_set_ip_adapter_image(sdm_ctx_t* ctx, const uint8_t* image, int w, int h, float strength);
/* Token state for the sampling entries (context state like sd_set_vae_tiling): sdm_generate_image and sd_sample_latents — the host loop, its fused branches, the
 * device-resident sampler, inpaint / pix2pix variants, the CFG-pair exchange — hand `tokens` [ip_dim, n_tokens] to the cond branch and `uncond_tokens` to every other
 * branch (uncond, img_uncond; stable-diffusion.cpp:2829-2843), scaled by `strength` (0: the graphs of a context without the adapter).  In a graph of K branches per image
 * they form one [ip_dim, n_tokens, K] input, assembled once per trajectory.  tokens NULL clears.  uncond_tokens NULL: the projection of an all-zero embedding
 * (stable-diffusion.cpp:2206-2207; not zero when the projection's LayerNorm has a bias) — n_tokens must then be the projection's token count.  Every device group
 * (device_batch images of the request at a time) of a call uses the same tokens. */
SD_API bool sd_set_ip_adapter(sdm_ctx_t* ctx, const float* tokens, const float* uncond_tokens, int64_t n_tokens, float strength);
/* sd_ip_adapter_project of one CLIP image embedding [clip_dim] + sd_set_ip_adapter with the default uncond tokens, as the reference does; NULL clears */
SD_API bool sd_set_ip_adapter_embeds(sdm_ctx_t* ctx, const float* embeds, float strength);
/* sd_unet_forward_concat's arguments (c_concat NULL on a plain context) plus the image tokens ip_context [ip_dim, n_ip, ip_n] (ip_n 1 or a divisor of n) and ip_scale.
 * Every attn2 emits, behind its text attention, what block.hpp:382-389 emits: to_k_ip, to_v_ip, the attention of the same q onto them, SCALE, ADD.  ip_context NULL or
 * ip_scale 0: the graph of a context without the adapter */
SD_API bool sd_unet_forward_ip(sdm_ctx_t* ctx, const float* x, int w, int h, int c, int n, const float* timesteps, const float* context, int64_t ctx_dim, int64_t n_tokens,
                               int64_t ctx_n, const float* y, int64_t y_dim, int64_t y_n, const float* c_concat, int cc, int concat_n, const float* ip_context, int64_t n_ip,
                               int ip_n, float ip_scale, float* out);
/* the same forward WITHOUT the listed joint blocks — MMDiT::forward's skip_layers (mmdit.hpp:854-866), the extra evaluation of skip-layer guidance; MMDiT family only */
SD_API bool sd_unet_forward_skip_layers(sdm_ctx_t* ctx, const float* x, int w, int h, int c, int n, const float* timesteps, const float* context, int64_t ctx_dim,
                                        int64_t n_tokens, int64_t ctx_n, const float* y, int64_t y_dim, int64_t y_n, const int* skip_layers, int n_skip, float* out);
/* VAE decode_first_stage (stable-diffusion.cpp:3062-3078): latents [w,h,zc,n] (diffusion scale) -> rgb f32 [8w,8h,3,n] in [0,1] */
SD_API bool sd_vae_decode(sdm_ctx_t* ctx, const float* latents, int w, int h, int c, int n, float* out_rgb);
/* the same WITHOUT the host step of VAE::decode (vae.hpp:216-218: (x + 1) / 2 and the clamp): what the decoder graph wrote, [8w,8h,3,n] — with tiling on, the merged canvas.
 * sd_vae_decode is this call followed by that step (the reference also applies it once, to the merged result, never per tile) */
SD_API bool sd_vae_decode_raw(sdm_ctx_t* ctx, const float* latents, int w, int h, int c, int n, float* out);
/* VAE tiling: sd_tiling_params_t (include/stable-diffusion.h, `--vae-tiling`; sd_img_gen_params_t::vae_tiling_params), same fields, same order, same defaults
 * ({false, 0, 0, 0.5f, 0, 0}), + tile_batch (OURS): tiles decoded / encoded per graph compute, stacked along the batch dimension (GroupNorm and attention are per
 * sample, so a tile's arithmetic does not depend on its neighbours in the batch); 0 = the engine's default (DESIGN.md 1, row "VAE tiling").  Tile sizes follow
 * VAE::get_tile_sizes (src/model/vae/vae.hpp:89-116), tile counts / achieved overlap sd_tiling_calc_tiles (src/core/ggml_extend.hpp:691-739, non-circular branch),
 * tile order / positions / the shifted last tile process_tiles_2d (:823-951), the overlap blend sd_tensor_merge_2d (:771-821).  Not implemented: circular and
 * temporal tiling, extra_tiling_args. */
typedef struct {
    bool enabled;
    int tile_size_x, tile_size_y; /* latent cells; < 4 = the default 32 */
    float target_overlap;         /* clamped to [0, 0.5] */
    float rel_size_x, rel_size_y; /* (0, 1]: fraction of the latent size; > 1: tile count; wins over tile_size_* */
    int tile_batch;
} sdm_tiling_params_t;
SD_API void sdm_tiling_params_init(sdm_tiling_params_t* p);
/* context state like sd_use_tae (the reference keeps vae_tiling_params on its context too): honoured by sd_vae_decode(_raw), sd_vae_encode and, through them,
 * sdm_generate_image.  NULL or enabled == false: the untiled path, exactly as before.  Tiles are cropped on the host, run through the ordinary VAE graph
 * tile_batch at a time (one graph topology for every full batch) and blended ON THE DEVICE into a canvas that is read back once (the reference merges on the
 * host per tile); with tiling on, the encoder's Gaussian sample and latent scaling run on the merged moments (VAE::encode, vae.hpp:118-168) */
SD_API bool sd_set_vae_tiling(sdm_ctx_t* ctx, const sdm_tiling_params_t* params);
/* the tile plan alone (host arithmetic, for known-answer tests): small_w x small_h is the LATENT size (decode: of the input; encode: of the output),
 * encode_factor VAE::get_tile_sizes' encoding_factor (1 decode, 2 the image VAE's encode).  tile_size[2] / overlap[2]: latent cells per axis (x, y);
 * tiles: (x, y, dx, dy) per tile in processing order (y outer, x inner), all in latent cells — dx / dy are the first columns / rows of a shifted last tile
 * that the merge skips.  Returns the tile count (also when it exceeds tile_capacity: nothing beyond the capacity is written), -1 on bad arguments. */
SD_API int sd_tiling_plan(int small_w, int small_h, const sdm_tiling_params_t* params, float encode_factor, int* tile_size, int* overlap, int* tiles, int tile_capacity);
/* the tiling driver with the IDENTITY in place of the VAE (tile size / overlap in cells of the input, encode_factor 1): crops, tile batches, the device merge and
 * the read-back alone — [w,h,c,n] -> [w,h,c,n].  The ramps of overlapping tiles sum to 1, so the result equals the input up to rounding (partition-of-unity test) */
SD_API bool sd_tiling_blend(sdm_ctx_t* ctx, const float* in, int w, int h, int c, int n, float* out);
/* VAE encode — encode_first_stage (stable-diffusion.cpp:3042-3060): rgb f32 planar [w,h,3,n] in [0,1] -> diffusion latents [w/8,h/8,zc,n], SAMPLED from the encoder's diagonal
 * Gaussian with Philox(seed) like the reference (auto_encoder_kl.hpp:750-759) and scaled to the diffusion model's range; moments_out (optional) receives the graph's output
 * [w/8,h/8,2*zc,n] (mean | log-variance).  The encoder ("first_stage_model.encoder. ...", "first_stage_model.quant_conv. ...") is made on first use. */
SD_API bool sd_vae_encode(sdm_ctx_t* ctx, const float* rgb, int w, int h, int n, uint64_t seed, float* out_latents, float* moments_out);
/* sd_ctx_params_t::prediction: SDM_V_PRED switches the UNet families to CompVisVDenoiser's scalings (denoiser.hpp:1198-1205) in the host loop and the device-resident sampler */
SD_API bool sd_set_prediction(sdm_ctx_t* ctx, int prediction);
/* TAESD, the tiny autoencoder's decoder (src/model/vae/tae.hpp:123-183, 732-792; the reference's `--taesd`): the same latents -> rgb f32 [8w,8h,3,n], NOT clamped (the graph's
 * output is the image; the u8 stage clamps).  The module (parameters "tae.decoder.layers.<i>. ...", 4 latent channels, 16 for the DiT families) is made on first use;
 * sd_load_weights_prefixed(ctx, file, "tae.") loads a taesd checkpoint into it.  sd_use_tae(ctx, true): sdm_generate_image decodes with it instead of the KL-VAE. */
SD_API bool sd_tae_decode(sdm_ctx_t* ctx, const float* latents, int w, int h, int c, int n, float* out_rgb);
SD_API bool sd_use_tae(sdm_ctx_t* ctx, bool on);
/* sample(): init noise (Philox seed+b) -> Euler(-A) loop with CFG -> final latents [w,h,c,batch_count] */
SD_API bool sd_sample_latents(sdm_ctx_t* ctx, const sdm_img_gen_params_t* p, float* out_latents);
/* sdm_generate_image: sample + decode + uint8 RGB.  Caller frees with sdm_free_images (library callocs). */
SD_API bool sdm_generate_image(sdm_ctx_t* ctx, const sdm_img_gen_params_t* p, sdm_image_t** images_out, int* num_images_out);
SD_API void sdm_free_images(sdm_image_t* images, int num_images);

/* ---- step caches: the reference's `--cache-mode easycache` (DiT families), `ucache` (UNet families), `dbcache` / `taylorseer` / `cache-dit` (DiT families) and
 * `spectrum` (UNet and DiT families) ---------------------------------------------------------------------------------------------------------------------------------
 * sd_cache_params_t of include/stable-diffusion.h.  The condition-level caches (src/runtime/easycache.hpp, ucache.hpp, CacheDitConditionState of cache_dit.hpp,
 * sample-cache.cpp): a denoise step whose model output can be predicted from the previous computed step (output = input + (previous output - previous input)) is
 * not run.  dbcache, taylorseer and cache-dit are ONE such cache in the reference (the block-level CacheDitState is used nowhere by its sampler): they differ from
 * EasyCache in the metric only — the relative L1 change of the model input against a fixed threshold — and the three modes behave identically.  Spectrum
 * (src/runtime/spectrum.hpp) replaces whole denoise calls, on a schedule that does not depend on data, by a forecast from the last K denoised tensors.  The
 * state machines are restated in csrc/host/step_cache.hpp.  Mode values as in the reference's sd_cache_mode_t. */
enum sdm_cache_mode_t {
    SDM_CACHE_DISABLED   = 0,
    SDM_CACHE_EASYCACHE  = 1,
    SDM_CACHE_UCACHE     = 2,
    SDM_CACHE_DBCACHE    = 3,
    SDM_CACHE_TAYLORSEER = 4,
    SDM_CACHE_CACHE_DIT  = 5,
    SDM_CACHE_SPECTRUM   = 6
};
typedef struct {
    enum sdm_cache_mode_t mode;
    float reuse_threshold;       /* INFINITY = the mode's default (EasyCache 0.2, UCache 1.0); negative values count as 0 */
    float start_percent;         /* the cache may act on steps inside (start_percent, end_percent) of the trajectory; an invalid range disables it */
    float end_percent;
    float error_decay_rate;      /* UCache, clamped to [0, 1] */
    bool use_relative_threshold; /* UCache */
    bool reset_error_on_compute; /* UCache */
} sdm_cache_params_t;
SD_API void sdm_cache_params_init(sdm_cache_params_t* p); /* sd_cache_params_init: DISABLED, INFINITY, 0.15, 0.95, 1.0, true, true */
/* Context state like sd_set_vae_tiling; NULL or SDM_CACHE_DISABLED turns it off (the sampler paths are then exactly the uncached ones).  Honoured by
 * sd_sample_latents / sdm_generate_image with every sample method, on the host loop and on the device-resident sampler.  A mode that does not fit the model family
 * or an invalid percent range is NOT an error: the trajectory runs uncached like the reference's, and sd_step_cache_status says why.  One decision per device
 * group: with device_batch > 1 the three means run over the whole group (the reference samples one image at a time).  false (sd_last_error): a NaN parameter.
 * Refused at sampling time (sd_last_error): an armed cache together with skip-layer guidance, or with a CFG-pair exchange (sd_set_pair_exchange*). */
SD_API bool sd_set_step_cache(sdm_ctx_t* ctx, const sdm_cache_params_t* params);
/* The options of the modes 3 .. 6 that change a trajectory in the reference (its warm-up, max-cached-steps, max-continuous-cached-steps, steps-computation-mask and
 * taylorseer_* options change none: DESIGN.md section 0). */
typedef struct {
    int Fn_compute_blocks;         /* > 0: the threshold is scaled by clamp(1 + 0.02 * (Fn - 8), 0.5, 2) */
    int Bn_compute_blocks;         /* > 0: ... and by clamp(1 - 0.03 * Bn, 0.5, 1) */
    float residual_diff_threshold; /* a step is skipped while sum |prev_in - in| / (sum |prev_in| + 1e-6) stays under the scaled threshold */
} sdm_cache_dit_params_t;
typedef struct {
    float w;            /* weight of the Chebyshev forecast; 1 - w goes to the first-order extrapolation */
    int m;              /* polynomial degree, 0 .. 15; the history holds K = max(m + 1, 6) denoised tensors */
    float lam;          /* ridge term */
    int window_size;    /* every floor(window)-th call after warm-up is computed; the window starts here ... */
    float flex_window;  /* ... and grows by this much with every computed call after warm-up */
    int warmup_steps;   /* denoise calls that are always computed */
    float stop_percent; /* calls from (int)(stop_percent * steps) on are always computed */
} sdm_spectrum_params_t;
SD_API void sdm_cache_dit_params_init(sdm_cache_dit_params_t* p); /* 8, 0, 0.08 */
SD_API void sdm_spectrum_params_init(sdm_spectrum_params_t* p);   /* 0.40, 3, 1.0, 2, 0.50, 4, 0.9 */
/* sd_set_step_cache plus the two extensions; a NULL extension means its defaults (so does sd_set_step_cache with one of the modes 3 .. 6).  false (sd_last_error): a
 * NaN parameter, or m outside 0 .. 15.  The CacheDIT modes on a UNet family, an invalid percent range (checked for every mode, though the CacheDIT window is fixed
 * at 15 % .. 95 % of the ladder and Spectrum has no window) and Spectrum with the two CFG++ sample methods run uncached, and sd_step_cache_status says why. */
SD_API bool sd_set_step_cache_ex(sdm_ctx_t* ctx, const sdm_cache_params_t* params, const sdm_cache_dit_params_t* cache_dit, const sdm_spectrum_params_t* spectrum);
/* one record per denoise call (model evaluation request of the sampler) of the last trajectory — the last device group of the last sd_sample_latents */
typedef struct {
    int step;            /* what the sampler handed the denoise call: i + 1, negated for the first stage of the two-stage methods (never cached) */
    float sigma;
    bool active;         /* inside the cache's sigma window */
    bool skipped;        /* the model was not run: outputs were rebuilt from the stored differences */
    float input_change;  /* mean |input - previous computed input| (0 when not measured); CacheDIT modes: the relative residual diff, as `rate` */
    float output_change; /* mean |output - previous computed output| of the anchor condition (computed steps; 0 when there was no previous output) */
    float output_norm;   /* mean |output| of the anchor condition (computed steps) */
    float rate;          /* the estimated output change of this step the decision added (0 when no decision was due) */
    float accumulated;   /* EasyCache: cumulative change rate, UCache: accumulated error — after adding `rate`, before any reset; CacheDIT modes: the accumulated residual diff */
    float threshold;     /* the effective threshold `accumulated` was compared with */
} sdm_cache_step_t; /* Spectrum: active = past warm-up and before the stop call, skipped = forecast instead of computed, the metric fields 0 */
SD_API int sd_step_cache_trace(sdm_ctx_t* ctx, sdm_cache_step_t* out, int capacity); /* returns the record count (also with capacity 0); at most `capacity` are written */
SD_API const char* sd_step_cache_status(sdm_ctx_t* ctx);                             /* "easycache" / "ucache" / "dbcache" / "taylorseer" / "cache-dit" / "spectrum" when the last trajectory was armed, else why not */
/* whether the device-resident sampler's two cache passes run as the backend's HIP kernels (true) or as the host restatement of a backend without those exports (false);
 * an MI355X backend that lacks the exports is an error at sampling time, never a quiet fall-back */
SD_API bool sd_step_cache_device_passes(sdm_ctx_t* ctx);
SD_API float sd_t_to_sigma(sdm_ctx_t* ctx, float t);                                 /* the context's denoiser (what the caches' percent_to_sigma goes through) */
/* The two device passes of the device-resident sampler's cache on caller memory (tests): uploads, runs probe and record through the path the sampler uses (the
 * backend's exports "ggml_backend_mi355x_step_cache_probe" / "_record", or the host restatement on a backend without them), reads back.  in / prev_in / prev_out:
 * [n, nb]; out / diff_out: [n, k, nb] with k = 1 or 2.  stats[0] = sum |in * c_in - prev_in|, stats[1] = sum |out_0 - prev_out| (prev_out NULL: never written, 0),
 * stats[2] = sum |out_0|; diff_out_j = out_j - in, prev_in_out = in, prev_out_out = out_0. */
SD_API bool sd_step_cache_kernels(sdm_ctx_t* ctx, const float* in, const float* out, const float* prev_in, const float* prev_out, int64_t n, int k, int nb, float c_in,
                                  float* stats, float* diff_out, float* prev_in_out, float* prev_out_out);
/* the CacheDIT modes' probe the same way ("ggml_backend_mi355x_step_cache_probe_rel"): sums[0] = sum |in * c_in - prev_in|, sums[1] = sum |prev_in| over n floats */
SD_API bool sd_step_cache_kernels_rel(sdm_ctx_t* ctx, const float* in, const float* prev_in, int64_t n, float c_in, float* sums);
/* Spectrum for tests.  schedule: predicted[i] = 1 when denoise call i of a trajectory of n_calls single-stage steps is forecast.  weights: the k history weights
 * for the taus of the k stored calls (oldest first) and the tau of the call to forecast.  kernels: the forecast itself on caller memory — hist [k][n] oldest first —
 * through the path the device sampler uses ("ggml_backend_mi355x_spectrum_predict", or the host restatement on a backend without it). */
SD_API bool sd_spectrum_schedule(const sdm_spectrum_params_t* params, int n_calls, uint8_t* predicted);
SD_API bool sd_spectrum_weights(const sdm_spectrum_params_t* params, const float* taus, int k, float tau_at, float* weights);
SD_API bool sd_spectrum_kernels(sdm_ctx_t* ctx, const float* hist, int k, int64_t n, const float* weights, float w, float* out);

/* ---- latent previews while sampling: the reference's sd_set_preview_callback / `--preview proj|tae|vae` (include/stable-diffusion.h:152-157, 441-446) -----------
 * The callback receives an RGB picture of the trajectory at denoise calls of sd_sample_latents / sdm_generate_image, on the host loop (every sample method) and on
 * the device-resident sampler: `step` is what the sampler hands the denoise call (i + 1, negated for the first stage of the two-stage methods), frames are
 * frame_count images of the current device group, is_noisy tells the model input (x * c_in, before the model call; not delivered on a Spectrum forecast call) from
 * the denoised prediction (after the inpainting blend; also delivered on calls a step cache skipped or forecast).  Frames belong to the engine and are valid only
 * during the callback.  PROJ: the family's latent -> RGB projection at latent resolution (w/8 x h/8); TAE / VAE: the latent decoded by TAESD / the first-stage
 * decoder (sd_set_vae_tiling honoured) at full resolution.  The byte stages run as HIP kernels on the MI355X backend (kernels/preview.hip); on the device-resident
 * sampler only the bytes (decode modes: and the small latent) cross to the host, and every delivered preview is one stream synchronisation.
 * Differences from the reference: the state is per context (the reference's is process-global, hence the sdm_ prefix); `interval` is honoured — a call is
 * previewed when abs(step) % max(interval, 1) == 0 — where the reference stores it and never reads it (interval 1 is its behaviour).
 * With no callback installed every sampler path is exactly the one without previews.  Refused at sampling time (sd_last_error): an installed preview on the
 * device-resident sampler together with a CFG-pair exchange (sd_set_pair_exchange*). */
enum sdm_preview_t { SDM_PREVIEW_NONE, SDM_PREVIEW_PROJ, SDM_PREVIEW_TAE, SDM_PREVIEW_VAE };   /* preview_t's values */
typedef void (*sdm_preview_cb_t)(int step, int frame_count, sdm_image_t* frames, bool is_noisy, void* data);
SD_API bool sdm_set_preview_callback(sdm_ctx_t* ctx, sdm_preview_cb_t cb, int mode, int interval, bool denoised, bool noisy, void* data); /* cb NULL or mode NONE: off */
SD_API int  sdm_preview_first_image(sdm_ctx_t* ctx);   /* inside a callback: batch index of frames[0] (device groups) */
/* inside a callback: the f32 latent [w, h, c, frame_count] the frames were made from, BEFORE in_scale (the noisy preview of the device-resident sampler hands x with
 * in_scale = c_in; everywhere else in_scale is 1).  Copies at most `capacity` floats; returns the latent's float count (0 outside a callback) */
SD_API int64_t sdm_preview_latent(sdm_ctx_t* ctx, float* out, int64_t capacity, float* in_scale);
SD_API bool sdm_set_preview_projection(sdm_ctx_t* ctx, const float* proj /* [c][3] */, const float* bias /* [3] or NULL */, int c); /* NULL proj: back to the family table */
SD_API bool sdm_latent_preview(sdm_ctx_t* ctx, const float* latents, int w, int h, int c, int n, float in_scale, uint8_t* out_rgb); /* the PROJ pass on caller memory, through the path the sampler uses */
SD_API bool sdm_planar_to_u8(sdm_ctx_t* ctx, const float* chw, int w, int h, int n, uint8_t* out_rgb);                               /* the decode modes' byte stage, same */
SD_API bool sdm_preview_device_passes(sdm_ctx_t* ctx);  /* like sd_step_cache_device_passes */

/* ---- host-side sampler pieces exposed for known-answer tests ---- */
SD_API void sd_philox_randn(uint64_t seed, uint32_t offset, uint32_t n, float* out); /* rng_philox.hpp:101-122 */
SD_API void sd_philox_uint32(uint64_t seed, uint32_t offset, uint32_t n, uint32_t* out /* 4*n words */); /* the integer stage alone: philox4_32, rng_philox.hpp:63-77 */
SD_API int sd_get_sigmas(int steps, float* out /* steps+1 */);                       /* denoiser.hpp:32-54 + stable-diffusion.cpp:173-186 */
/* CFG-pair split across two GPUs (the cond / uncond evaluations of src/runtime/guidance.cpp:149-179 on two devices):
 * with an exchange installed, the device-resident trajectory (device_sampler) evaluates ONE branch per step on this context — branch 0 = cond,
 * 1 = uncond — writes weight * eps (weight = cfg on branch 0, 1 - cfg on branch 1) to a device buffer and calls `exchange` once per step with
 * that buffer's DEVICE address, its f32 element count and the hipStream_t the producer graph was enqueued on (NULL on host backends).  The
 * callee sums the two ranks' buffers in place (one all-reduce, e.g. RCCL over one xGMI link) ordered on that stream, and returns false on
 * failure.  Nothing is copied to the host.  fn = NULL restores the single-device CFG pair. */
typedef bool (*sd_pair_exchange_fn)(void* device_eps, int64_t count, void* stream, void* user);
SD_API void sd_set_pair_exchange(sdm_ctx_t* ctx, sd_pair_exchange_fn fn, void* user, int branch);
/* Native RCCL form of the exchange (csrc/host/rccl_exchange.cpp): librccl.so is loaded with dlopen, no torch involved.  Rank 0 of a pair makes the
 * 128-byte unique id and ships it to its partner by any means (a file, a socket, torch.distributed in the tests); both create a 2-rank
 * communicator bound to HIP device `device` and install it: the engine then issues ONE in-place ncclAllReduce(SUM, f32) of its eps buffer per
 * sampler step on the backend stream (replaces the reference's host-side guidance.cpp:149-179 when cond and uncond run on two GPUs). */
SD_API bool sd_rccl_get_unique_id(void* id128);
SD_API void* sd_rccl_comm_create(int device, int nranks, int rank, const void* id128); /* NULL on failure (sd_rccl_last_error) */
SD_API void sd_rccl_comm_destroy(void* comm);
SD_API bool sd_set_pair_exchange_rccl(sdm_ctx_t* ctx, void* comm, int branch); /* comm = NULL removes the exchange */
SD_API const char* sd_rccl_last_error(void);
SD_API void sd_set_guidance(sdm_ctx_t* ctx, float guidance); /* FLUX distilled-guidance input (default 3.5, stable-diffusion.h guidance.distilled_guidance) */
/* the host sampler's classifier-free-guidance combine on n floats: out = uncond + scale * (cond - uncond), three separately rounded f32 operations like
 * sd::guidance::ClassifierFreeGuidance::forward on sd::Tensor<float> (src/runtime/guidance.cpp:171) — bit-exact against that code compiled into oracle/_ref */
SD_API void sd_cfg_combine(const float* cond, const float* uncond, int64_t n, float scale, float* out);
/* ---- c_concat and three-conditioning guidance of the inpaint / pix2pix UNets: the reference's mask_image + inpaint versions, guidance.img_cfg, ref_images[0] of the
 * UNet edit models.  Context state like sd_set_vae_tiling, read by sd_sample_latents / sdm_generate_image on the host loop and the device-resident sampler.
 * concat [w,h,cc,n] (latent cells; cc = sd_concat_channels): n = 1 shared by the batch (the reference's case) or n = batch_count (device groups take their slice);
 * NULL clears.  img_uncond_concat NULL derives the reference's default (stable-diffusion.cpp:5145, 5168, 5173): inpaint keeps the mask channel and zeroes the masked
 * latent, pix2pix is all zeros.  cond and uncond both see `concat`; the third condition is uncond's text with `img_uncond_concat` (:5236-5237, 5265-5266, 5273).
 * Branches exactly as resolve_guidance (:4237-4255): uncond runs iff img_cfg != txt_cfg (img_cfg 1: today's txt_cfg != 1), img_uncond iff img_cfg != 1; img_cfg
 * INFINITY (the default) = 1.  On a plain context a value other than 1 is accepted and ignored (the reference's warning is left in sd_last_error).  The combine has
 * ClassifierFreeGuidance::forward's three forms (guidance.cpp:162-176), every operation a separately rounded f32, left to right:
 *   three branches iu + img * (u - iu) + txt * (c - u);  img_uncond only iu + txt * (c - iu);  uncond only u + txt * (c - u).
 * The CFG++ methods' denoised_uncond takes img_uncond first, then uncond, then cond (:2880-2883).  A variant context sampled without a concat condition fails.
 * Refused at sampling time (sd_last_error): a third branch together with adaptive projected guidance, with an armed step cache (two-branch concat sampling with a
 * cache works) or with a CFG-pair exchange.  The device-resident sampler assembles the model input and combines the three predictions in one launch each on the
 * MI355X backend (k_model_input / k_guidance3, include/ggml-mi355x.h options fuse_model_input / fuse_guidance3). */
SD_API bool sd_set_concat_condition(sdm_ctx_t* ctx, const float* concat, const float* img_uncond_concat, int w, int h, int cc, int n);
SD_API bool sd_set_img_cfg(sdm_ctx_t* ctx, float img_cfg);
/* the combine on n floats; uncond or img_uncond NULL selects the two-prediction forms — bit-exact against guidance.cpp compiled into oracle/_ref */
SD_API void sd_cfg_combine3(const float* cond, const float* uncond, const float* img_uncond, int64_t n, float txt_cfg, float img_cfg, float* out);
/* The device-resident sampler's two glue stages on caller memory, as the graphs the sampler emits through the backend it uses (tests).
 *   model input: x [w,h,c,nb], concat [w,h,cc,k] (shared: row j is branch j's) or [w,h,cc,k*nb] (concat_per_image) -> xin_out [w,h,c+cc,k*nb]: plane p < c of model
 *                image b*k + j is x[b] * c_in, plane p >= c is the concat row (MUL -> RESHAPE -> REPEAT -> RESHAPE, [REPEAT,] CONCAT; k = 1: MUL, [REPEAT,] CONCAT)
 *   guidance:    e3 [per,3,nb] (cond, uncond, img_uncond adjacent per image), per = w*h*c -> guided_out [per,nb], the six nodes of the three-term combine with the
 *                scales read from the step's scalar tensor on the device
 * Either stage is skipped when its output pointer is NULL. */
SD_API bool sd_guidance_kernels(sdm_ctx_t* ctx, const float* x, float c_in, const float* concat, int w, int h, int c, int cc, int k, int nb, bool concat_per_image,
                                float* xin_out, const float* e3, float txt_cfg, float img_cfg, float* guided_out);
/* pixels -> the concat condition (prepare_image_generation_latents, stable-diffusion.cpp:4986-5010, 5127-5173, 5197-5203): rgb planar [w,h,3] in [0,1], mask [w,h].
 * INPAINT: the mask is rounded (sd::ops::round: halves away from zero), latent mask = interpolate(NearestMax) to w/8 x h/8, masked image (1 - mask) * (rgb - 0.5) + 0.5
 * encoded with sd_vae_encode(seed); concat_out [w/8,h/8,5] = latent mask | masked latent; img_uncond_concat_out = latent mask | zeros; denoise_mask_out [w/8,h/8] =
 * the 3x3 / stride 1 / pad 1 max-pool of the latent mask; init_latent_out = the encoded unmasked image (sdm_img_gen_params_t::init_latent / denoise_mask).
 * PIX2PIX: concat_out [w/8,h/8,4] = the encoded image (mask ignored, may be NULL), img_uncond_concat_out zeros, no denoise mask (not written).
 * Optional outputs may be NULL. */
SD_API bool sd_make_inpaint_condition(sdm_ctx_t* ctx, const float* rgb, const float* mask, int w, int h, uint64_t seed, float* concat_out, float* img_uncond_concat_out,
                                      float* denoise_mask_out, float* init_latent_out);
SD_API bool sd_latent_mask(const float* mask, int w, int h, float* out /* [w/8,h/8] */);   /* the two mask stages alone, for known-answer tests */
SD_API bool sd_mask_max_pool3(const float* in, int w, int h, float* out);
/* the pixel stage of sdm_generate_image on caller memory: planar CHW floats in [0, 1] -> interleaved RGB bytes (src/runtime/preprocessing.hpp:27-60); for the
 * bit-exact test against that header compiled into oracle/_ref */
SD_API void sd_planar_rgb_to_u8(const float* chw, int width, int height, uint8_t* out);
/* the host sampler loop (sigma ladder, initial noise, scalings / timestep per step, ancestral step, update, Philox noise order) on one image of n floats with
 * a synthetic model, denoised = x / (1 + sigma) + 0.01 * sigma: family 0 CompVis (SD1.x / SDXL), 1 discrete flow (SD3.x), 2 FLUX flow; method = sdm_sample_method_t;
 * eta INFINITY = the method's default; aux: optional 5 floats per step (c_skip, c_out, c_in, t, sigma).  Returns the ladder length, -1 on bad arguments.  For the
 * bit-exact tests against the reference's src/runtime/denoiser.hpp compiled into oracle/_ref (tests/test_host_logic.py). */
SD_API int sd_sample_synthetic(int family, int steps, int image_seq_len, int64_t n, uint64_t seed, int method, float eta, float* out, float* aux);
/* the same with a scheduler (sdm_scheduler_t; SDM_SCHEDULER_COUNT = the default) and any implemented method; aux receives 5 floats per MODEL CALL in call order (at most aux_calls
 * of them); returns the number of model calls, or -1 */
SD_API int sd_sample_synthetic2(int family, int steps, int image_seq_len, int64_t n, uint64_t seed, int method, int scheduler, float eta, float* out, float* aux, int aux_calls);
/* sigma ladder of a denoiser family (0 CompVis SD1.x, 1 discrete flow, 2 FLUX flow, 3 CompVis with the SDXL Align-Your-Steps table) under a scheduler; shift <= 0: the family's default;
 * returns the count (steps + 1) or -1 for a scheduler that is not implemented */
SD_API int sd_get_sigmas_sched(int family, int scheduler, int steps, int image_seq_len, float shift, float* out);
/* adaptive projected guidance over `steps` successive calls on one image of n floats (cond / uncond / out: [steps][n]); for the bit-exact test against guidance.cpp */
SD_API void sd_apg_sequence(const float* cond, const float* uncond, int64_t n, int steps, float scale, float eta, float momentum, float norm_threshold,
                            float norm_threshold_smoothing, float* out);
/* AutoEncoderKL::set_conv2d_scale (src/model/vae/auto_encoder_kl.hpp:708-717): every Conv2d of the VAE computes conv(x * s) / s + bias.  SDXL contexts start with
 * s = 1/32 — what the reference sets when no external VAE is given (src/stable-diffusion.cpp:1477-1485; `--vae` with a fixed VAE -> call this with 1) */
SD_API bool sd_set_vae_conv2d_scale(sdm_ctx_t* ctx, float scale); /* false (sd_last_error) for a non-finite or non-positive scale; loading a file under the
                                                                     "first_stage_model" prefix (= --vae) resets an SDXL context to scale 1 like the reference */
SD_API int sd_get_flux_sigmas(int steps, int image_seq_len, float* out /* steps+1 */); /* FluxScheduler, denoiser.hpp:726-782 */
SD_API int sd_gen_flux_pe(int h, int w, int patch_size, int context_len, const int* axes_dim, int n_axes, float theta, float* out); /* Rope::gen_flux_pe; returns floats written */
SD_API int sd_get_flow_sigmas(int steps, float shift, float* out /* steps+1 */);    /* DiscreteFlowDenoiser, denoiser.hpp:1239-1283 (t = 1000*sigma) */
SD_API float sd_sigma_to_t(float sigma);                                             /* denoiser.hpp:1140-1165 */

/* Node-by-node evaluation hook: the reference's sd_graph_eval_callback_t / sd_set_backend_eval_callback (include/stable-diffusion.h:442-447; used by the
 * imatrix collector, src/runtime/imatrix.cpp:39-100,180).  With a callback installed every graph a context computes goes through
 * sdm_backend_graph_compute_with_eval_callback, which restates sd_backend_graph_compute_with_eval_callback (src/core/ggml_extend_backend.cpp:466-509)
 * statement for statement: the callback is asked about every node (ask = true); the graph is cut BEHIND each node it wants, the slice is handed to the
 * backend as a SUB-GRAPH VIEW built exactly like sd_ggml_graph_view (:449-463: nodes + i0, n_leafs 0, leafs NULL, size 0, uid 0, the PARENT's use_counts /
 * visited_hash_set), computed async + synchronised, then the callback sees the node again (ask = false) and may read it and its sources; returning false
 * stops the graph (GGML_STATUS_ABORTED).  The sdm_ prefix keeps the names apart from the reference's own symbols. */
struct ggml_tensor;
struct ggml_cgraph;
struct ggml_backend;
typedef bool (*sdm_graph_eval_callback_t)(struct ggml_tensor* t, bool ask, void* user_data);
SD_API void sdm_set_backend_eval_callback(sdm_graph_eval_callback_t cb, void* user_data);
SD_API int sdm_backend_graph_compute_with_eval_callback(struct ggml_backend* backend, struct ggml_cgraph* gf, sdm_graph_eval_callback_t cb, void* user_data); /* enum ggml_status */

/* Graph topology as text, for the node-for-node comparison with the graphs the REFERENCE's own builders emit (tests/test_ref_graphs.py; the reference side is
 * oracle/ref_graphs_wrap.cpp -> oracle/_ref/libref_graphs.so, which calls this same function on its graphs).  One line per leaf ("L <j> type ne nb flags name")
 * and per node ("N <i> OP type ne nb op_params flags sources view_src@offset name"), sources as n<i> / l<j>.  Returns the bytes needed incl. the
 * terminating 0 (call with cap 0 to size the buffer).  sdm_set_graph_capture(1): every graph an engine context computes is described just before it is
 * submitted and kept until the next one; 2: described and NOT computed (the call fails with "graph captured, compute skipped": topology of full-size models
 * without the arithmetic); sdm_last_graph_description copies it out. */
SD_API size_t sdm_graph_describe(struct ggml_cgraph* gf, char* buf, size_t cap);
SD_API void sdm_set_graph_capture(int on);
SD_API size_t sdm_last_graph_description(char* buf, size_t cap);

/* ---- timing / introspection ---- */
typedef struct {
    double last_sample_ms;  /* denoise loop wall time of the last sd_sample_latents / sdm_generate_image */
    double last_decode_ms;  /* VAE decode wall time */
    int64_t unet_calls;     /* graph computes issued */
    int64_t graph_nodes;    /* nodes in the last UNet graph */
    size_t compute_buffer_bytes;
    size_t weight_bytes;
    /* cumulative HOST time of the denoiser runner since context creation (ms): graph construction, gallocr allocation, and
     * uploads + graph_compute (which contains the device time on the synchronous path, only the enqueue cost on the device-resident path) */
    double host_build_ms, host_alloc_ms, host_submit_ms;
    int64_t graph_cache_hits; /* denoiser calls that replayed the cached graph (same shapes as the previous call) instead of rebuilding it */
    int64_t steps_skipped;    /* denoise steps the step cache (sd_set_step_cache) did not run in the last sd_sample_latents / sdm_generate_image, over all device groups; after a call that failed it counts the groups that had finished only */
} sd_stats_t;
SD_API void sd_get_stats(sdm_ctx_t* ctx, sd_stats_t* out);
/* ---- text encoders + conditioner --------------------------------------------------------
 * CLIP text towers (src/model/te/clip.hpp) and the T5 encoder (src/model/te/t5.hpp) as graphs on the same backend, and the
 * conditioner composition of src/conditioning/conditioner.hpp (SD1.x/SDXL :414-544, SD3 :842-1015, FLUX :1209-1297).  Inputs are
 * TOKEN IDS (+ per-token prompt weights): the reference's vocabularies are not part of its source drop, so tokenisation stays with
 * the caller.  Encoders are created on first use with synthetic weights (weight_seed); sd_load_weights overwrites them when the file
 * names "cond_stage_model.*" / "text_encoders.*" tensors. */
typedef struct {
    const int32_t* ids;
    const float* weights; /* NULL = all 1.0 */
    int n;                /* multiple of the chunk length: 77 for CLIP and SD3's T5, 256 for FLUX's T5 */
} sd_token_list_t;
SD_API bool sd_text_encoders_init(sdm_ctx_t* ctx);
/* which: 0 = clip_l (ViT-L/14), 1 = clip_g (ViT-bigG/14).  CLIPTextModelRunner::compute (clip.hpp:562-583): hidden states
 * [hidden, n_tokens] after layer n_layer - clip_skip (clip_skip <= 0: all layers), or with return_pooled the final-LN'd row
 * max_token_idx (times text_projection for bigG).  Returns floats written, -1 on error. */
SD_API int64_t sd_clip_forward(sdm_ctx_t* ctx, int which, const int32_t* ids, int n_tokens, int max_token_idx, bool return_pooled, int clip_skip, float* out,
                               int64_t out_capacity);
SD_API int64_t sd_t5_forward(sdm_ctx_t* ctx, const int32_t* ids, int n_tokens, float* out, int64_t out_capacity); /* T5Runner::compute, t5.hpp:452-461 */
SD_API int sd_t5_relative_position_buckets(int q_len, int k_len, int32_t* out /* q_len*k_len */);                 /* t5.hpp:463-530 */
/* token ids -> SDCondition.  crossattn_ne = {ctx_dim, n_tokens}; pass NULL output pointers to query the sizes first.  clip_g / t5
 * are ignored by families that do not own them (SD1.x and SDXL derive the bigG ids from clip_l like the reference). */
SD_API bool sd_get_learned_condition(sdm_ctx_t* ctx, const sd_token_list_t* clip_l, const sd_token_list_t* clip_g, const sd_token_list_t* t5, int clip_skip,
                                     int width, int height, bool zero_out_masked, float* crossattn_out, int64_t crossattn_capacity, int64_t* crossattn_ne,
                                     float* vector_out, int64_t vector_capacity, int64_t* vector_n);


#ifdef __cplusplus
}
#endif
#endif
