// preview.hpp — latent previews while sampling: the reference's sd_set_preview_callback / `--preview proj|tae|vae` (include/stable-diffusion.h:152-157, 441-446;
// preview_image, src/stable-diffusion.cpp:2279-2409; preview_latent_video, src/runtime/latent-preview.h:401-459) as per-context state of this engine.
//   - the latent -> RGB projection tables of the four families this engine runs (published constants: ComfyUI's latent formats; the SD3 one from Stability's
//     sd3_impls.py), held here like sampler.hpp holds the GITS / AYS ladders
//   - the host restatement of the two byte stages (kernels/preview.hip), operation for operation: used on a backend without the exports
//   - the schedule rule and the context state
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "sd-mi355x.h"

struct PreviewTable {
    int channels;
    const float (*proj)[3];
    const float* bias;
};

// SD1.x / SD2.x
static const float PREVIEW_SD_PROJ[4][3] = {
    {0.337366f, 0.216344f, 0.257386f}, {0.165636f, 0.386828f, 0.046994f}, {-0.267803f, 0.237036f, 0.223517f}, {-0.178022f, -0.200862f, -0.678514f}};
static const float PREVIEW_SD_BIAS[3] = {-0.017478f, -0.055834f, -0.105825f};
// SDXL
static const float PREVIEW_SDXL_PROJ[4][3] = {
    {0.258303f, 0.277640f, 0.329699f}, {-0.299701f, 0.105446f, 0.014194f}, {0.050522f, 0.186163f, -0.143257f}, {-0.211938f, -0.149892f, -0.080036f}};
static const float PREVIEW_SDXL_BIAS[3] = {0.144381f, -0.033313f, 0.007061f};
// SD3.x (zero bias)
static const float PREVIEW_SD3_PROJ[16][3] = {
    {-0.0645f, 0.0177f, 0.1052f}, {0.0028f, 0.0312f, 0.0650f},  {0.1848f, 0.0762f, 0.0360f},    {0.0944f, 0.0360f, 0.0889f},
    {0.0897f, 0.0506f, -0.0364f}, {-0.0020f, 0.1203f, 0.0284f}, {0.0855f, 0.0118f, 0.0283f},    {-0.0539f, 0.0658f, 0.1047f},
    {-0.0057f, 0.0116f, 0.0700f}, {-0.0412f, 0.0281f, -0.0039f}, {0.1106f, 0.1171f, 0.1220f},   {-0.0248f, 0.0682f, -0.0481f},
    {0.0815f, 0.0846f, 0.1207f},  {-0.0120f, -0.0055f, -0.0867f}, {-0.0749f, -0.0634f, -0.0456f}, {-0.1418f, -0.1457f, -0.1259f}};
static const float PREVIEW_SD3_BIAS[3] = {0.0f, 0.0f, 0.0f};
// FLUX.1
static const float PREVIEW_FLUX_PROJ[16][3] = {
    {-0.041168f, 0.019917f, 0.097253f},  {0.028096f, 0.026730f, 0.129576f},  {0.065618f, -0.067950f, -0.014651f}, {-0.012998f, -0.014762f, 0.081251f},
    {0.078567f, 0.059296f, -0.024687f},  {-0.015987f, -0.003697f, 0.005012f}, {0.033605f, 0.138999f, 0.068517f},  {-0.024450f, -0.063567f, -0.030101f},
    {-0.040194f, -0.016710f, 0.127185f}, {0.112681f, 0.088764f, -0.041940f}, {-0.023498f, 0.093664f, 0.025543f},  {0.082899f, 0.048320f, 0.007491f},
    {0.075712f, 0.074139f, 0.081965f},   {-0.143501f, 0.018263f, -0.136138f}, {-0.025767f, -0.082035f, -0.040023f}, {-0.111849f, -0.055589f, -0.032361f}};
static const float PREVIEW_FLUX_BIAS[3] = {0.024600f, -0.006937f, -0.008089f};

// preview_image's choice by version and channel count (stable-diffusion.cpp:2325-2349) for the model families of sd-mi355x.h
inline PreviewTable preview_family_table(int model) {
    switch (model) {
        case SD_MODEL_SD15:
        case SD_MODEL_SD15_TINY: return {4, PREVIEW_SD_PROJ, PREVIEW_SD_BIAS};
        case SD_MODEL_SDXL:
        case SD_MODEL_SDXL_TINY: return {4, PREVIEW_SDXL_PROJ, PREVIEW_SDXL_BIAS};
        case SD_MODEL_FLUX_DEV:
        case SD_MODEL_FLUX_TINY:
        case SD_MODEL_FLUX_WIDE1:
        case SD_MODEL_FLUX_WIDE8: return {16, PREVIEW_FLUX_PROJ, PREVIEW_FLUX_BIAS};
        default: return {16, PREVIEW_SD3_PROJ, PREVIEW_SD3_BIAS};  // the MMDiT families
    }
}

constexpr int PREVIEW_MAX_CHANNELS = 128;  // the kernel's table capacity

// ---- the two byte stages on host memory, in the kernels' operation order (this library is built without contraction: every operation rounds on its own) ----
// x [plane, c, n] -> out [n * plane][3]; proj NULL (c == 3): pass-through, no bias; bias NULL: zeros
inline bool latent_preview_host(const float* x, int64_t plane, int c, int64_t n, float in_scale, const float* proj, const float* bias, uint8_t* out) {
    if (!x || !out || plane < 1 || n < 1 || c < 1 || c > PREVIEW_MAX_CHANNELS || (!proj && c != 3)) return false;
    const bool scaled = in_scale != 1.0f;
    for (int64_t im = 0; im < n; ++im)
        for (int64_t i = 0; i < plane; ++i) {
            const float* src = x + im * c * plane + i;
            float acc[3]     = {0.0f, 0.0f, 0.0f};
            if (proj) {
                for (int d = 0; d < c; ++d) {
                    const float v = scaled ? src[(int64_t)d * plane] * in_scale : src[(int64_t)d * plane];
                    for (int k = 0; k < 3; ++k) {
                        const float m = v * proj[3 * d + k];
                        acc[k]        = acc[k] + m;
                    }
                }
                for (int k = 0; k < 3; ++k) acc[k] = acc[k] + (bias ? bias[k] : 0.0f);
            } else {
                for (int k = 0; k < 3; ++k) acc[k] = scaled ? src[(int64_t)k * plane] * in_scale : src[(int64_t)k * plane];
            }
            for (int k = 0; k < 3; ++k) {
                const float h = acc[k] * 0.5f;
                float m       = h + 0.5f;
                m             = (0.0f < m) ? m : 0.0f;
                m             = (m < 1.0f) ? m : 1.0f;
                const float s = m * 255.0f;
                out[(im * plane + i) * 3 + k] = (uint8_t)s;
            }
        }
    return true;
}
// x [plane, 3, n] -> out [n * plane][3]: preprocessing_float_to_u8 (src/runtime/preprocessing.hpp:27-35) behind v = x * in_mul + in_add; NaN -> 0
inline bool planar_to_u8_host(const float* x, int64_t plane, int64_t n, float in_mul, float in_add, uint8_t* out) {
    if (!x || !out || plane < 1 || n < 1) return false;
    const bool affine = in_mul != 1.0f || in_add != 0.0f;
    for (int64_t im = 0; im < n; ++im)
        for (int k = 0; k < 3; ++k) {
            const float* src = x + (im * 3 + k) * plane;
            for (int64_t i = 0; i < plane; ++i) {
                float v = src[i];
                if (affine) {
                    const float h = v * in_mul;
                    v             = h + in_add;
                }
                uint8_t byte;
                if (!(v > 0.0f))
                    byte = 0;
                else if (v >= 1.0f)
                    byte = 255;
                else {
                    const float s = v * 255.0f;
                    const float r = s + 0.5f;
                    byte          = (uint8_t)r;
                }
                out[(im * plane + i) * 3 + k] = byte;
            }
        }
    return true;
}

// a denoise call with sampler step s (i + 1, negated for the first stage of the two-stage methods) is previewed when |s| % max(interval, 1) == 0.  Interval 1 is the
// reference's behaviour (it stores the interval and never reads it, src/core/util.cpp:633, 653); larger values are this engine's extension
inline bool preview_due(int step, int interval) { return std::abs(step) % (interval > 1 ? interval : 1) == 0; }

struct PreviewState {
    sdm_preview_cb_t cb = nullptr;
    void* user          = nullptr;
    int mode            = SDM_PREVIEW_NONE;
    int interval        = 1;
    bool denoised = true, noisy = false;
    std::vector<float> custom_proj;  // [c][3] when sdm_set_preview_projection installed one
    float custom_bias[3] = {0.0f, 0.0f, 0.0f};
    int custom_c         = 0;
    std::vector<uint8_t> bytes;    // the frames handed to the callback
    std::vector<float> staging;    // read-backs of the device-resident sampler, decode outputs of the host route
    bool on() const { return cb != nullptr && mode != SDM_PREVIEW_NONE; }
    bool wants(int step, bool is_noisy) const { return on() && (is_noisy ? noisy : denoised) && preview_due(step, interval); }
};
