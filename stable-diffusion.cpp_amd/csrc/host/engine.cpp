// engine.cpp — host driver of the hot path + the C ABI declared in include/sd-mi355x.h.
//
// Mirrors (re-designed, not transcribed):
//   GGMLRunner::compute / execute_graph      src/core/ggml_extend.hpp:3151-3210, 2767-2930
//   StableDiffusionGGML::sample + denoise    src/stable-diffusion.cpp:2509-2926
//   sample_euler_ancestral / sample_euler    src/runtime/denoiser.hpp:1513-1546, 1582-1597
//   ClassifierFreeGuidance::forward          src/runtime/guidance.cpp:149-179
//   decode_first_stage / VAE::decode         src/stable-diffusion.cpp:3062-3078, src/model/vae/vae.hpp:170-222
//   sdm_generate_image batch loop                src/stable-diffusion.cpp:5664-5721
//
// Like the reference, the graph is rebuilt for every model call; unlike it, `device_batch`
// images are denoised together in ONE graph (N>1 is our extension, F6) — per-image results are defined
// as those of independent batch-1 runs with seeds seed+b.
#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "ggml.h"
#include "models.hpp"
#include "conditioner.hpp"
#include "clip_vision.hpp"
#include "sampler.hpp"
#include "step_cache.hpp"
#include "preview.hpp"
#include "model_io.hpp"
#include "torch_ckpt_io.hpp"
#include "name_conversion.hpp"
#include "sd-mi355x.h"

using namespace sdmi;

static thread_local std::string g_last_error;
static void set_error(const std::string& e) {
    g_last_error = e;
    fprintf(stderr, "[sd-mi355x] error: %s\n", e.c_str());
}
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// host post-processing of whole image batches (clamp / uint8 conversion of 6.3 M floats for 8 x 512x512) on a few threads
template <typename Fn>
static void parallel_chunks(size_t n, Fn&& fn, size_t min_parallel = (1u << 16)) {
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const size_t T    = n < min_parallel ? 1 : std::min<size_t>(hw, n);
    if (T == 1) {
        fn((size_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    const size_t step = (n + T - 1) / T;
    for (size_t t = 0; t < T; ++t) {
        const size_t b = t * step, e = std::min(n, b + step);
        if (b < e) th.emplace_back([&fn, b, e]() { fn(b, e); });
    }
    for (auto& t : th) t.join();
}

// ---------------------------------------------------------------------------------------------------
// synthetic weights: deterministic per tensor name, N(0, 1/sqrt(fan_in)) weights, small biases,
// norm scales around 1
// ---------------------------------------------------------------------------------------------------
static inline uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t hash_name(const std::string& s, uint64_t seed) {
    uint64_t h = 1469598103934665603ull ^ seed;
    for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
    return h;
}
static void fill_normal(float* dst, int64_t n, uint64_t seed, float mean, float std) {
    const int nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<unsigned>(std::thread::hardware_concurrency(), 16u), n / 65536));
    auto work          = [&](int tid) {
        const int64_t chunk = (n + nthreads - 1) / nthreads;
        const int64_t i0 = tid * chunk, i1 = std::min<int64_t>(n, i0 + chunk);
        // counter-based: value i depends only on (seed, i/2) so the result is thread-count independent
        for (int64_t i = i0 & ~1ll; i < i1; i += 2) {
            uint64_t s  = seed + (uint64_t)(i / 2) * 0x632BE59BD9B4E019ull;
            uint64_t r1 = splitmix64(s), r2 = splitmix64(s);
            const float u1 = ((float)(r1 >> 40) + 0.5f) * (1.0f / 16777216.0f);
            const float u2 = ((float)(r2 >> 40) + 0.5f) * (1.0f / 16777216.0f);
            const float m  = sqrtf(-2.0f * logf(u1));
            const float a = m * cosf(6.2831853f * u2), b = m * sinf(6.2831853f * u2);
            if (i >= i0 && i < i1) dst[i] = mean + std * a;
            if (i + 1 >= i0 && i + 1 < i1) dst[i + 1] = mean + std * b;
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& t : th) t.join();
}

// ---------------------------------------------------------------------------------------------------
// node-by-node evaluation hook (include/sd-mi355x.h): restates src/core/ggml_extend_backend.cpp:449-509 and src/core/util.cpp:638-668
// ---------------------------------------------------------------------------------------------------
static sdm_graph_eval_callback_t g_eval_cb = nullptr;
static void* g_eval_cb_data                = nullptr;

static ggml_cgraph graph_view(ggml_cgraph* parent, int i0, int i1) {  // sd_ggml_graph_view
    ggml_cgraph v;
    v.size             = 0;
    v.n_nodes          = i1 - i0;
    v.n_leafs          = 0;
    v.nodes            = parent->nodes + i0;
    v.grads            = nullptr;
    v.grad_accs        = nullptr;
    v.leafs            = nullptr;
    v.use_counts       = parent->use_counts;
    v.visited_hash_set = parent->visited_hash_set;
    v.order            = parent->order;
    v.uid              = 0;
    return v;
}

extern "C" void sdm_set_backend_eval_callback(sdm_graph_eval_callback_t cb, void* user_data) {
    g_eval_cb      = cb;
    g_eval_cb_data = user_data;
}

extern "C" int sdm_backend_graph_compute_with_eval_callback(ggml_backend* backend, ggml_cgraph* gf, sdm_graph_eval_callback_t cb, void* user_data) {
    if (cb == nullptr) return (int)ggml_backend_graph_compute(backend, gf);
    enum ggml_status status = GGML_STATUS_SUCCESS;
    const int n_nodes       = ggml_graph_n_nodes(gf);
    bool stopped            = false;
    for (int j0 = 0; j0 < n_nodes; ++j0) {
        ggml_tensor* t = ggml_graph_node(gf, j0);
        bool need      = cb(t, true, user_data);
        int j1         = j0;
        while (!need && j1 < n_nodes - 1) {
            t    = ggml_graph_node(gf, ++j1);
            need = cb(t, true, user_data);
        }
        ggml_cgraph gv = graph_view(gf, j0, j1 + 1);
        status         = ggml_backend_graph_compute_async(backend, &gv);
        if (status != GGML_STATUS_SUCCESS) break;
        ggml_backend_synchronize(backend);
        if (need && !cb(t, false, user_data)) {
            stopped = true;
            break;
        }
        j0 = j1;
    }
    ggml_backend_synchronize(backend);
    if (stopped && status == GGML_STATUS_SUCCESS) status = GGML_STATUS_ABORTED;
    return (int)status;
}

// ---------------------------------------------------------------------------------------------------
// graph topology as text (include/sd-mi355x.h: sdm_graph_describe)
// ---------------------------------------------------------------------------------------------------
static std::string describe_graph(ggml_cgraph* gf) {
    std::unordered_map<const ggml_tensor*, std::string> ref;
    std::vector<const ggml_tensor*> leafs;
    auto leaf_ref = [&](const ggml_tensor* t) -> const std::string& {
        auto it = ref.find(t);
        if (it != ref.end()) return it->second;
        leafs.push_back(t);
        return ref[t] = "l" + std::to_string(leafs.size() - 1);
    };
    for (int i = 0; i < gf->n_nodes; ++i) ref[gf->nodes[i]] = "n" + std::to_string(i);
    if (gf->leafs)
        for (int j = 0; j < gf->n_leafs; ++j) leaf_ref(gf->leafs[j]);
    std::string nodes;
    char line[1024];
    for (int i = 0; i < gf->n_nodes; ++i) {
        const ggml_tensor* t = gf->nodes[i];
        int n = snprintf(line, sizeof(line), "N %d %s %s ne=%lld,%lld,%lld,%lld nb=%zu,%zu,%zu,%zu p=", i, ggml_op_name(t->op), ggml_type_name(t->type), (long long)t->ne[0],
                         (long long)t->ne[1], (long long)t->ne[2], (long long)t->ne[3], t->nb[0], t->nb[1], t->nb[2], t->nb[3]);
        nodes.append(line, n);
        int last = -1;
        for (int k = 0; k < (int)(sizeof(t->op_params) / sizeof(int32_t)); ++k)
            if (t->op_params[k] != 0) last = k;
        for (int k = 0; k <= last; ++k) {
            n = snprintf(line, sizeof(line), k ? ",%d" : "%d", t->op_params[k]);
            nodes.append(line, n);
        }
        n = snprintf(line, sizeof(line), " f=%d s=", t->flags);
        nodes.append(line, n);
        bool any = false;
        for (int k = 0; k < GGML_MAX_SRC; ++k) {
            if (!t->src[k]) continue;
            if (any) nodes += ',';
            nodes += std::to_string(k) + ":" + leaf_ref(t->src[k]);
            any = true;
        }
        if (!any) nodes += '-';
        nodes += " v=";
        if (t->view_src) {
            nodes += leaf_ref(t->view_src) + "@" + std::to_string(t->view_offs);
        } else {
            nodes += '-';
        }
        nodes += " name=";
        nodes += t->name;
        nodes += '\n';
    }
    std::string out;
    for (size_t j = 0; j < leafs.size(); ++j) {
        const ggml_tensor* t = leafs[j];
        const int n = snprintf(line, sizeof(line), "L %zu %s ne=%lld,%lld,%lld,%lld nb=%zu,%zu,%zu,%zu f=%d name=%s\n", j, ggml_type_name(t->type), (long long)t->ne[0], (long long)t->ne[1],
                               (long long)t->ne[2], (long long)t->ne[3], t->nb[0], t->nb[1], t->nb[2], t->nb[3], t->flags, t->name);
        out.append(line, n);
    }
    return out + nodes;
}
static int g_graph_capture = 0;  // 1: describe every graph before it is submitted; 2: describe it and do NOT compute (topology of full-size models on a CPU box)
static std::string g_last_graph;
extern "C" size_t sdm_graph_describe(ggml_cgraph* gf, char* buf, size_t cap) {
    const std::string d = describe_graph(gf);
    if (buf && cap > 0) {
        const size_t n = std::min(cap - 1, d.size());
        memcpy(buf, d.data(), n);
        buf[n] = 0;
    }
    return d.size() + 1;
}
extern "C" void sdm_set_graph_capture(int on) {
    g_graph_capture = on;
    if (!on) g_last_graph.clear();
}
extern "C" size_t sdm_last_graph_description(char* buf, size_t cap) {
    if (buf && cap > 0) {
        const size_t n = std::min(cap - 1, g_last_graph.size());
        memcpy(buf, g_last_graph.data(), n);
        buf[n] = 0;
    }
    return g_last_graph.size() + 1;
}

// ---------------------------------------------------------------------------------------------------
// Runner: weights residency + per-call graph lifecycle
// ---------------------------------------------------------------------------------------------------
struct HostInput {
    ggml_tensor* t;
    const void* data;
    size_t nbytes;
};

struct Runner {
    ggml_backend_t backend        = nullptr;
    ParamStore ps;
    ggml_backend_buffer_t weights = nullptr;
    ggml_gallocr_t galloc         = nullptr;
    size_t graph_size             = 102400;  // UNET_GRAPH_SIZE (unet.hpp:14)
    int64_t calls                 = 0;
    int64_t last_nodes            = 0;
    double build_ms = 0, alloc_ms = 0, submit_ms = 0;  // cumulative host time: graph construction, gallocr, uploads + graph_compute call
    const void* last_res_data = nullptr;  // where the last compute's result tensor lies in the compute buffer: valid until this runner places another graph (a decode preview
    size_t last_res_bytes     = 0;        // converts the image there, behind the graph on the backend stream, instead of reading it back as f32)

    ~Runner() {
        drop_cache();
        if (galloc) ggml_gallocr_free(galloc);
        if (weights) ggml_backend_buffer_free(weights);
    }

    bool alloc_weights(uint64_t seed) {
        weights = ggml_backend_alloc_ctx_tensors(ps.ctx, backend);
        if (!weights) return false;
        ggml_backend_buffer_set_usage(weights, GGML_BACKEND_BUFFER_USAGE_WEIGHTS);
        // graph-topology tests of the full-size models (tests/test_ref_graphs.py) build and describe graphs without computing them: the 8-12 B parameter
        // tables are allocated (untouched pages) and left unfilled
        if (getenv("SDCPP_SKIP_WEIGHT_INIT")) return true;
        std::vector<float> tmp;
        std::vector<uint8_t> conv;
        double t_fill = 0, t_up = 0;
        for (auto& sp : ps.specs) {
            const int64_t n = ggml_nelements(sp.tensor);
            if ((int64_t)tmp.size() < n) tmp.resize(n);  // grow only: every element is overwritten below
            const uint64_t s = hash_name(sp.name, seed);
            const double t0  = now_ms();
            switch (sp.kind) {
                case InitKind::WEIGHT: fill_normal(tmp.data(), n, s, 0.f, 1.0f / sqrtf((float)sp.fan_in)); break;
                case InitKind::BIAS: fill_normal(tmp.data(), n, s, 0.f, 0.02f); break;
                case InitKind::NORM_SCALE: fill_normal(tmp.data(), n, s, 1.f, 0.05f); break;
                case InitKind::ZERO: std::fill(tmp.begin(), tmp.begin() + n, 0.f); break;
            }
            const double t1 = now_ms();
            upload_f32(sp.tensor, tmp.data(), conv);
            t_fill += t1 - t0;
            t_up += now_ms() - t1;
        }
        if (getenv("SDCPP_INIT_TIMING")) fprintf(stderr, "[sd-mi355x] synthetic init: %zu tensors, fill %.0f ms, convert + upload %.0f ms\n", ps.specs.size(), t_fill, t_up);
        return true;
    }

    void upload_f32(ggml_tensor* t, const float* src, std::vector<uint8_t>& scratch) {
        const int64_t n = ggml_nelements(t);
        if (t->type == GGML_TYPE_F32) {
            ggml_backend_tensor_set(t, src, 0, n * 4);
            return;
        }
        scratch.resize(ggml_nbytes(t));
        // model_loader.cpp:168-202; rows are independent, so big tensors convert on a few threads (the software f32 -> f16 / q8_0 / q4_0
        // row encoders run at a few ns per element: 4 s of a 7 s SD1.5 context creation, minutes for a 12 B-parameter FLUX)
        const int64_t rows = n / t->ne[0], per_row = t->ne[0];
        const ggml_type ty = t->type;
        uint8_t* dst       = scratch.data();
        if (ty == GGML_TYPE_F16 || ty == GGML_TYPE_BF16) {
            // elementwise encodings: convert flat ranges (conv kernels have ne0 = 3, a row-wise walk would pay one call per 3 elements)
            parallel_chunks((size_t)n, [&](size_t i0, size_t i1) {
                if (ty == GGML_TYPE_F16)
                    ggml_fp32_to_fp16_row(src + i0, (ggml_fp16_t*)dst + i0, (int64_t)(i1 - i0));
                else
                    ggml_fp32_to_bf16_row(src + i0, (ggml_bf16_t*)dst + i0, (int64_t)(i1 - i0));
            }, 1 << 20);
        } else if (n < (1 << 20)) {
            ggml_quantize_chunk(ty, src, dst, 0, rows, per_row, nullptr);
        } else {
            parallel_chunks((size_t)rows, [&](size_t r0, size_t r1) { ggml_quantize_chunk(ty, src, dst, (int64_t)r0 * per_row, (int64_t)(r1 - r0), per_row, nullptr); }, 2);
        }
        ggml_backend_tensor_set(t, scratch.data(), 0, scratch.size());
    }

    // ---- one cached graph (OUR host-side optimisation; the reference rebuilds and re-allocates per call, ggml_extend.hpp:2767-2930):
    // consecutive calls with the same signature (shapes + flags) reuse the built graph and its gallocr placement — only the inputs are
    // uploaded again.  Building the 2570-node SD1.5 UNet graph and placing it costs 1.5–2.3 ms of host time per step, which on the
    // synchronous path sits between two device steps.  Any other graph allocated from this runner's gallocr invalidates the entry.
    std::string cache_sig;
    ggml_context* cache_ctx = nullptr;
    ggml_cgraph* cache_gf   = nullptr;
    ggml_tensor* cache_res  = nullptr;
    std::vector<HostInput> cache_inputs, cache_builtin;
    int64_t cache_hits = 0;
    void drop_cache() {
        if (cache_ctx) ggml_free(cache_ctx);
        cache_ctx = nullptr;
        cache_gf  = nullptr;
        cache_res = nullptr;
        cache_inputs.clear();
        cache_builtin.clear();
        cache_sig.clear();
    }

    // build -> alloc -> upload inputs -> compute -> download   (ggml_extend.hpp:2767-2930)
    // out == nullptr: nothing is downloaded and nothing waits — inputs go through set_tensor_async and the graph through
    // graph_compute_async on the backend's stream, so the host can build the next graph while this one runs (device-resident sampler)
    // sig / ptrs: non-empty sig enables the cached graph; ptrs are this call's host buffers in the order `build` declares its inputs
    template <typename BuildFn>
    bool compute(BuildFn&& build, float* out, size_t out_bytes, const std::string& sig = std::string(), const std::vector<const void*>& ptrs = {}) {
        ggml_context* cctx = nullptr;
        ggml_cgraph* gf    = nullptr;
        ggml_tensor* res   = nullptr;
        std::vector<HostInput> local_inputs, local_builtin;  // builtin: the runner's own two leaves (uploaded with the inputs, not part of the caller's pointer list)
        std::vector<HostInput>* inputs = &local_inputs;
        const bool cacheable = !sig.empty();
        double t_s = now_ms();
        if (cacheable && cache_ctx && cache_sig == sig && cache_inputs.size() == ptrs.size()) {
            cctx = cache_ctx;
            gf   = cache_gf;
            res  = cache_res;
            for (size_t i = 0; i < ptrs.size(); ++i) cache_inputs[i].data = ptrs[i];
            inputs = &cache_inputs;
            ++cache_hits;
        } else {
            drop_cache();  // whatever is placed next reuses the gallocr buffer
            ggml_init_params ip{0, nullptr, true};
            cctx = ggml_init(ip);
            gf   = ggml_new_graph_custom(cctx, graph_size, false);
            GraphCtx g;
            g.ctx            = cctx;
            g.backend        = backend;
            const double t_b = now_ms();
            res              = build(g, local_inputs);
            // GGMLRunner::get_compute_graph (ggml_extend.hpp:2040-2064) only NAMES the last node; it does not flag it GGML_TENSOR_FLAG_OUTPUT (round 6: found
            // by comparing with the graph the reference's own runner emits, tests/test_ref_graphs.py) and appends two built-in one-element leaves
            ggml_set_name(res, "ggml_runner_final_result_tensor");
            ggml_build_forward_expand(gf, res);
            {
                ggml_tensor* one = ggml_new_tensor_1d(cctx, GGML_TYPE_F32, 1);  // prepare_build_in_tensor_before / _after, ggml_extend.hpp:2023-2036
                ggml_set_name(one, "ggml_runner_build_in_tensor:one");
                ggml_set_input(one);  // set_backend_tensor_data marks what it uploads (ggml_extend.hpp:3090-3095)
                ggml_tensor* zero_int = ggml_new_tensor_1d(cctx, GGML_TYPE_I32, 1);
                ggml_set_name(zero_int, "ggml_runner_build_in_tensor:zero_int");
                ggml_set_input(zero_int);
                ggml_build_forward_expand(gf, one);
                ggml_build_forward_expand(gf, zero_int);
                static const float one_v    = 1.f;
                static const int32_t zero_v = 0;
                local_builtin.push_back(HostInput{one, &one_v, sizeof(one_v)});
                local_builtin.push_back(HostInput{zero_int, &zero_v, sizeof(zero_v)});
            }
            const double t_a = now_ms();
            build_ms += t_a - t_b;
            if (!galloc) galloc = ggml_gallocr_new(ggml_backend_get_default_buffer_type(backend));
            const bool ok = ggml_gallocr_alloc_graph(galloc, gf);
            t_s           = now_ms();
            alloc_ms += t_s - t_a;
            if (!ok) {
                set_error("compute buffer allocation failed");
                ggml_free(cctx);
                return false;
            }
            if (cacheable) {
                bool same = ptrs.size() == local_inputs.size();
                for (size_t i = 0; same && i < ptrs.size(); ++i) same = ptrs[i] == local_inputs[i].data;
                if (same) {  // the caller's pointer list matches what the builder declared: safe to replay with new pointers
                    cache_sig    = sig;
                    cache_ctx    = cctx;
                    cache_gf     = gf;
                    cache_res    = res;
                    cache_inputs = local_inputs;
                    inputs       = &cache_inputs;
                    cache_builtin = local_builtin;
                }
            }
        }
        const bool keep  = cctx == cache_ctx;
        const bool async = out == nullptr;
        if (g_graph_capture) g_last_graph = describe_graph(gf);
        if (g_graph_capture == 2) {
            set_error("graph captured, compute skipped (sdm_set_graph_capture(2))");
            if (keep)
                drop_cache();
            else
                ggml_free(cctx);
            return false;
        }
        for (const std::vector<HostInput>* list : {(const std::vector<HostInput>*)inputs, (const std::vector<HostInput>*)(keep ? &cache_builtin : &local_builtin)})
            for (auto& in : *list) {
                if (!in.t->data && !in.t->buffer) continue;  // a leaf nothing reads is not placed
                if (async)
                    ggml_backend_tensor_set_async(backend, in.t, in.data, 0, in.nbytes);
                else
                    ggml_backend_tensor_set(in.t, in.data, 0, in.nbytes);
            }
        // GGMLRunner::compute routes through the eval-callback variant whenever a callback is installed (ggml_extend.hpp:2857-2860)
        const enum ggml_status st = g_eval_cb ? (enum ggml_status)sdm_backend_graph_compute_with_eval_callback(backend, gf, g_eval_cb, g_eval_cb_data)
                                    : async   ? ggml_backend_graph_compute_async(backend, gf)
                                              : ggml_backend_graph_compute(backend, gf);
        if (st != GGML_STATUS_SUCCESS) {
            set_error(std::string("graph compute failed: ") + ggml_status_to_string(st));
            if (keep)
                drop_cache();
            else
                ggml_free(cctx);
            return false;
        }
        submit_ms += now_ms() - t_s;  // synchronous path: includes the device time of the graph
        if (!async) {
            if (ggml_nbytes(res) != out_bytes) {
                set_error("output size mismatch");
                if (keep)
                    drop_cache();
                else
                    ggml_free(cctx);
                return false;
            }
            ggml_backend_tensor_get(res, out, 0, out_bytes);
        }
        last_nodes     = gf->n_nodes;
        last_res_data  = res->data;
        last_res_bytes = ggml_nbytes(res);
        ++calls;
        if (!keep) ggml_free(cctx);
        return true;
    }
};

struct sdm_ctx_t {
    sdm_ctx_params_t params;
    ggml_backend_t backend = nullptr;
    Runner unet_runner, vae_runner;
    UNetModel unet;
    MMDiTModel mmdit;
    FluxModel flux;
    bool is_dit = false, is_flux = false;
    float guidance = 3.5f;
    float vae_conv2d_scale = 1.f;  // AutoEncoderKL::set_conv2d_scale (1/32 for SDXL, as the reference sets it without an external VAE)
    FluxFlowDenoiser flux_denoiser;
    VaeDecoder vae;
    CompVisDenoiser denoiser;
    DiscreteFlowDenoiser flow_denoiser;
    // the LATENT's channels (noise, x, what the VAE reads and writes): the family's, whatever the variant.  The UNet's first conv reads model_in_channels() =
    // latent_channels() + concat_channels() (9 on an inpaint UNet, 8 on a pix2pix one)
    int latent_channels() const { return is_flux ? 16 : (is_dit ? (int)mmdit.cfg.in_channels : unet.cfg.in_channels - concat_channels()); }
    int model_in_channels() const { return latent_channels() + concat_channels(); }
    int variant = SDM_UNET_PLAIN;  // sdm_unet_variant_t
    int concat_channels() const { return variant == SDM_UNET_INPAINT ? 5 : (variant == SDM_UNET_PIX2PIX ? 4 : 0); }
    // c_concat state (sd_set_concat_condition) and the image guidance scale (sd_set_img_cfg): context state like the VAE tiling parameters
    struct ConcatCondition {
        std::vector<float> concat, img_uncond;  // [w, h, cc, n] each; img_uncond is always filled (given or derived)
        int w = 0, h = 0, cc = 0, n = 0;
        bool set() const { return !concat.empty(); }
    };
    ConcatCondition concat_cond;
    float img_cfg = INFINITY;      // INFINITY = not set = 1 (resolve_guidance, stable-diffusion.cpp:4237-4240)
    std::string guidance_status;   // what sd_set_img_cfg had to say (a plain context ignores a scale other than 1, as the reference warns)
    int out_channels() const { return is_flux ? 16 : (is_dit ? (int)mmdit.cfg.out_channels : unet.cfg.out_channels); }
    // Denoiser::get_sigmas (denoiser.hpp:1046-1123): the scheduler sees this family's sigma_min / sigma_max / t_to_sigma.  sched = SCHED_COUNT: the family's own ladder
    std::vector<float> get_sigmas(uint32_t n, int image_seq_len, int sched = SCHED_COUNT) const {
        if (sched == SCHED_COUNT) sched = is_flux ? SCHED_FLUX : SCHED_DISCRETE;
        if (sched == SCHED_FLUX) return flux_denoiser.get_sigmas(n, image_seq_len);  // FluxScheduler needs only the sequence length
        if (is_flux) return scheduler_sigmas(sched, n, flux_denoiser.sigma_min(), flux_denoiser.sigma_max(), [&](float t) { return flux_denoiser.t_to_sigma(t); }, -1);
        if (is_dit) return scheduler_sigmas(sched, n, flow_denoiser.sigma_min(), flow_denoiser.sigma_max(), [&](float t) { return flow_denoiser.t_to_sigma(t); }, -1);
        const int ays = (params.model == SD_MODEL_SD15 || params.model == SD_MODEL_SD15_TINY) ? 0 : 1;  // AYSScheduler picks its table by version (denoiser.hpp:186-200)
        return scheduler_sigmas(sched, n, denoiser.sigma_min(), denoiser.sigma_max(), [&](float t) { return denoiser.t_to_sigma(t); }, ays);
    }
    void scalings(float sigma, float& c_skip, float& c_out, float& c_in) const {
        if (is_flux)
            flux_denoiser.scalings(sigma, c_skip, c_out, c_in);
        else if (is_dit)
            flow_denoiser.scalings(sigma, c_skip, c_out, c_in);
        else if (prediction == SDM_V_PRED) {  // CompVisVDenoiser::get_scalings (denoiser.hpp:1198-1205), sigma_data = 1
            const float sigma_data = 1.0f;
            c_skip = sigma_data * sigma_data / (sigma * sigma + sigma_data * sigma_data);
            c_out  = -sigma * sigma_data / std::sqrt(sigma * sigma + sigma_data * sigma_data);
            c_in   = 1.0f / std::sqrt(sigma * sigma + sigma_data * sigma_data);
        } else
            denoiser.scalings(sigma, c_skip, c_out, c_in);
    }
    int prediction = SDM_EPS_PRED;  // sd_ctx_params_t::prediction (stable-diffusion.h): the UNet families' parameterisation
    float sigma_to_t(float sigma) const { return is_flux ? sigma : (is_dit ? flow_denoiser.sigma_to_t(sigma) : denoiser.sigma_to_t(sigma)); }
    sd_stats_t stats{};
    std::vector<std::pair<std::string, ggml_tensor*>> all_tensors;
    // text encoders: built on first use (sd_text_encoders_init / sd_get_learned_condition / a checkpoint naming them)
    struct TextEncoders {
        Runner l_runner, g_runner, t5_runner;
        ClipTextModel clip_l, clip_g;
        T5Model t5;
        ConditionerSpec spec;
        Runner* runner(int which) { return which == 0 ? &l_runner : (which == 1 ? &g_runner : &t5_runner); }
    };
    std::unique_ptr<TextEncoders> te;
    // device-resident sampler state: the latent batch and the current step's noise live in one persistent buffer
    struct SamplerState {
        ggml_context* sctx        = nullptr;
        ggml_backend_buffer_t buf = nullptr;
        ggml_tensor *x = nullptr, *noise = nullptr, *eps = nullptr;
        int64_t W = 0, H = 0, C = 0, N = 0;
        // step cache (sd_set_step_cache), made only when a cache is armed: the recorded input / outputs of the last computed step, what the anchor saw the
        // step before, the stored differences and the three sums (+ 1 spare) the host reads back once per active step
        struct Cache {
            ggml_context* cctx        = nullptr;
            ggml_backend_buffer_t buf = nullptr;
            ggml_tensor *in = nullptr, *out = nullptr, *prev_in = nullptr, *prev_out = nullptr, *diff = nullptr, *stats = nullptr;
            int k = 0;
            uint64_t serial = 0;  // part of the recording / skip-step graphs' signatures: a cached graph never outlives the tensors it names
            ~Cache() {
                if (buf) ggml_backend_buffer_free(buf);
                if (cctx) ggml_free(cctx);
            }
        };
        std::unique_ptr<Cache> cache;
        // Spectrum (sd_set_step_cache mode 6), made only when it is armed: the ring of the last K denoised tensors (slot stride padded to a multiple of 4 floats so
        // every slot starts 16-byte aligned) and the tensor a computed step records its `denoised` in and a forecast is written to
        struct Spectrum {
            ggml_context* cctx        = nullptr;
            ggml_backend_buffer_t buf = nullptr;
            ggml_tensor *ring = nullptr, *denoised = nullptr;
            int K = 0;
            int64_t stride = 0;
            uint64_t serial = 0;
            ~Spectrum() {
                if (buf) ggml_backend_buffer_free(buf);
                if (cctx) ggml_free(cctx);
            }
        };
        std::unique_ptr<Spectrum> spectrum;
        // latent previews (sdm_set_preview_callback), made only when a denoised preview is installed: the tensor `denoised` passes through on the steps a preview is due,
        // and the runners of those capturing graphs — their own cached graph and compute buffer, so that the step graphs of the steps in between (and of every later
        // trajectory without previews) keep the cached graph, the buffer placement and the backend plan they had
        struct Preview {
            ggml_context* cctx        = nullptr;
            ggml_backend_buffer_t buf = nullptr;
            ggml_tensor* denoised     = nullptr;
            uint64_t serial = 0;
            Runner step_runner, skip_runner;
            ~Preview() {
                if (buf) ggml_backend_buffer_free(buf);
                if (cctx) ggml_free(cctx);
            }
        };
        std::unique_ptr<Preview> preview;
        // c_concat of an inpaint / pix2pix UNet (sd_set_concat_condition), made only for such trajectories: constant over the steps, uploaded once per trajectory
        struct Concat {
            ggml_context* cctx        = nullptr;
            ggml_backend_buffer_t buf = nullptr;
            ggml_tensor* t            = nullptr;
            uint64_t serial = 0;  // part of the step graphs' signatures: a cached graph never outlives the tensor it names
            ~Concat() {
                if (buf) ggml_backend_buffer_free(buf);
                if (cctx) ggml_free(cctx);
            }
        };
        std::unique_ptr<Concat> concat;
        ~SamplerState() {
            concat.reset();
            cache.reset();
            spectrum.reset();
            preview.reset();
            if (buf) ggml_backend_buffer_free(buf);
            if (sctx) ggml_free(sctx);
        }
    };
    std::unique_ptr<SamplerState> sstate;
    // CFG-pair split (sd_set_pair_exchange): this context computes one branch; the per-step sum with the partner is the caller's collective
    sd_pair_exchange_fn pair_fn = nullptr;
    void* pair_user             = nullptr;
    int pair_branch             = 0;
    Runner pair_runner;  // the sampler-update graph behind the exchange keeps its own cached graph + compute buffer
    // step caches (sd_set_step_cache; csrc/host/step_cache.hpp): the request, the runtime of the current / last trajectory, and the runner of the device-resident
    // sampler's skip-step graph (its own cached graph: alternating with the step graph must not rebuild either)
    sdm_cache_params_t cache_params{SDM_CACHE_DISABLED, INFINITY, 0.15f, 0.95f, 1.0f, true, true};
    sdm_cache_dit_params_t cache_dit_params{8, 0, 0.08f};
    sdm_spectrum_params_t spectrum_params{0.40f, 3, 1.0f, 2, 0.50f, 4, 0.9f};
    StepCacheRuntime step_cache;
    Runner skip_runner;
    // latent previews (sdm_set_preview_callback; csrc/host/preview.hpp): the request, and — made on the first PROJ preview of the host loop on a backend with the
    // byte-stage exports — the tensor the group's latent is uploaded to
    PreviewState preview;
    struct PreviewUpload {
        ggml_context* cctx        = nullptr;
        ggml_backend_buffer_t buf = nullptr;
        ggml_tensor* latent       = nullptr;
        ~PreviewUpload() {
            if (buf) ggml_backend_buffer_free(buf);
            if (cctx) ggml_free(cctx);
        }
    };
    std::unique_ptr<PreviewUpload> preview_upload;
    struct PreviewCurrent {  // while a callback runs: the batch index of frames[0] and where the latent behind the frames lies (host memory or a backend tensor)
        bool active         = false;
        int first_image     = 0;
        const float* host   = nullptr;
        ggml_tensor* dev    = nullptr;
        int64_t floats      = 0;
        float in_scale      = 1.0f;
    };
    PreviewCurrent preview_current;
    float t_to_sigma(float t) const { return is_flux ? flux_denoiser.t_to_sigma(t) : (is_dit ? flow_denoiser.t_to_sigma(t) : denoiser.t_to_sigma(t)); }
    // whether the request would arm a cache on this family (init_sample_cache_runtime's tests that do not need the ladder)
    // method: the resolved sample method (Spectrum does not serve the two CFG++ methods)
    bool step_cache_would_arm(int method) const {
        if (!StepCacheRuntime::has_valid_cache_percent_range(cache_params)) return false;
        if (cache_params.mode == SDM_CACHE_SPECTRUM) return !sample_method_needs_uncond(method);
        if (StepCacheRuntime::is_cachedit_mode(cache_params.mode)) return is_dit;
        return (cache_params.mode == SDM_CACHE_EASYCACHE && is_dit) || (cache_params.mode == SDM_CACHE_UCACHE && !is_dit);
    }
    void step_cache_begin_trajectory(const std::vector<float>& sigmas, int method) {
        step_cache.init(&cache_params, is_dit, !is_dit, [this](float t) { return t_to_sigma(t); }, sigmas, &cache_dit_params, &spectrum_params,
                        sample_method_needs_uncond(method));
    }
    std::vector<float> pe_cache;  // FLUX rotary table of the last (h, w, n_tokens)
    int pe_h = 0, pe_w = 0;
    int64_t pe_tokens = 0;
    // KL-VAE encoder (auto_encoder_kl.hpp:276-366), made on first sd_vae_encode: the reference builds it unless vae_decode_only is set (stable-diffusion.cpp:1467-1474)
    Runner vae_enc_runner;
    VaeEncoder vae_enc;
    bool vae_enc_ready = false;
    // TAESD (tae.hpp): the tiny decoder next to the KL-VAE, made on first use (sd_tae_decode / sd_use_tae) like the reference makes it when a taesd file is given
    Runner tae_runner;
    TaeDecoder tae;
    bool tae_ready = false, tae_for_images = false;
    // VAE tiling (sd_set_vae_tiling): the parameters, and per direction (0 decode, 1 encode) the device-resident state of the last tiled call
    sdm_tiling_params_t tiling{false, 0, 0, 0.5f, 0.f, 0.f, 0};
    struct TileState {
        ggml_context* sctx        = nullptr;
        ggml_backend_buffer_t buf = nullptr;
        ggml_gallocr_t merge_galloc = nullptr;
        ggml_tensor* canvas = nullptr;                  // [W, H, C_out, N]: zeroed per call, blended into by the merge graphs, read back once
        ggml_tensor* store[2] = {nullptr, nullptr};     // the tile graph's result [TW, TH, C_out, N * k]: full batches / the short last batch
        ggml_tensor *wx = nullptr, *wy = nullptr;       // ramp vectors of every tile, [TW, 1, 1, T] and [1, TH, 1, T] (they depend on the plan only)
        std::string key;
        uint64_t serial = 0;  // part of the tile graph's signature: a cached graph never outlives the store tensor it copies into
        ~TileState() {
            if (merge_galloc) ggml_gallocr_free(merge_galloc);
            if (buf) ggml_backend_buffer_free(buf);
            if (sctx) ggml_free(sctx);
        }
    };
    std::unique_ptr<TileState> tstate[3];  // decode, encode, sd_tiling_blend
    // IP-Adapter (sd_ip_adapter_init): to_k_ip / to_v_ip of every attn2 and the image projection, in a weight buffer of their own — the resident weights stay untouched
    Runner ip_runner;
    ImageProjModel ip_proj;
    Resampler ip_resampler;  // the "plus" adapters' projection: the context holds one of the two (ip_plus)
    bool ip_plus = false;
    bool ip_ready = false;
    int64_t ip_dim = 0, ip_clip_dim = 0, ip_num_tokens = 0;
    // sd_set_ip_adapter: the image tokens of the sampling entries, [ip_dim, ip_set_n] each — `ip_tokens` for the cond branch, `ip_uncond` for every other branch
    // (uncond, img_uncond: stable-diffusion.cpp:2829-2843); empty = no adapter in the samplers
    std::vector<float> ip_tokens, ip_uncond;
    int64_t ip_set_n  = 0;
    float ip_strength = 0.f;
    bool ip_active() const { return ip_ready && ip_set_n > 0 && ip_strength != 0.f; }
    // K rows for a model batch whose K branches per image are adjacent (cond first, or `first_uncond` on the uncond rank of a CFG-pair exchange): [ip_dim, ip_set_n, K]
    std::vector<float> ip_rows(int K, bool first_uncond = false) const {
        std::vector<float> r;
        for (int j = 0; j < K; ++j) {
            const std::vector<float>& t = (j == 0 && !first_uncond) ? ip_tokens : ip_uncond;
            r.insert(r.end(), t.begin(), t.end());
        }
        return r;
    }
    // the tokens of the forward the host loop is about to run (HostDenoise sets it around its calls; sd_unet_forward / _concat carry no token arguments)
    struct IpCall {
        const float* data = nullptr;
        int ip_n          = 0;
    } ip_call;
    // CLIP vision tower (sd_clip_vision_init / sd_load_clip_vision): parameters in a weight buffer of their own
    Runner cv_runner;
    ClipVisionModel clip_vision;
    bool cv_ready = false;
    std::vector<Runner*> runners() {
        std::vector<Runner*> v{&unet_runner, &vae_runner};
        if (ip_ready) v.push_back(&ip_runner);
        if (cv_ready) v.push_back(&cv_runner);
        if (tae_ready) v.push_back(&tae_runner);
        if (vae_enc_ready) v.push_back(&vae_enc_runner);
        if (te) {
            if (te->spec.has_l) v.push_back(&te->l_runner);
            if (te->spec.has_g) v.push_back(&te->g_runner);
            if (te->spec.has_t5) v.push_back(&te->t5_runner);
        }
        return v;
    }
    ~sdm_ctx_t() {
        // runners free their buffers in their destructors; the backend must outlive them
    }
};

// ---------------------------------------------------------------------------------------------------
extern "C" {

const char* sd_last_error(void) { return g_last_error.c_str(); }

bool sd_load_backend(const char* path) { return ggml_backend_load(path) != nullptr; }
int sd_device_count(void) { return (int)ggml_backend_dev_count(); }
const char* sd_device_name(int i) {
    ggml_backend_dev_t d = ggml_backend_dev_get(i);
    return d ? ggml_backend_dev_name(d) : nullptr;
}
const char* sd_device_description(int i) {
    ggml_backend_dev_t d = ggml_backend_dev_get(i);
    return d ? ggml_backend_dev_description(d) : nullptr;
}

void sdm_ctx_params_init(sdm_ctx_params_t* p) {
    memset(p, 0, sizeof(*p));
    p->backend              = nullptr;
    p->model                = SD_MODEL_SD15;
    p->wtype                = SDM_TYPE_F16;
    p->diffusion_flash_attn = false;
    p->vae_decode_only      = true;
    p->weight_seed          = 1234;
    p->n_threads            = -1;
}
void sdm_sample_params_init(sdm_sample_params_t* p) {  // stable-diffusion.cpp:3650-3667
    memset(p, 0, sizeof(*p));
    p->txt_cfg       = 7.0f;
    p->scheduler     = SDM_SCHEDULER_COUNT;  // resolved per model and method at sampling time (sd_get_default_scheduler)
    p->sample_method = SDM_SAMPLE_METHOD_COUNT;  // resolved per family at sampling time (sd_get_default_sample_method)
    p->sample_steps  = 20;
    p->eta           = INFINITY;
    p->flow_shift    = INFINITY;  // the family's default (stable-diffusion.cpp:3665, 3106-3115)
    p->apg_eta         = 1.0f;    // AdaptiveProjectedGuidanceParams defaults (guidance.h:21-26): all neutral = plain classifier-free guidance
    p->slg_layer_start = 0.01f;   // stable-diffusion.cpp:3655-3658
    p->slg_layer_end   = 0.2f;
}
void sdm_img_gen_params_init(sdm_img_gen_params_t* p) {  // stable-diffusion.cpp:3710-3731
    memset(p, 0, sizeof(*p));
    sdm_sample_params_init(&p->sample_params);
    p->width       = 512;
    p->height      = 512;
    p->seed        = 42;
    p->batch_count = 1;
    p->decode      = true;
    p->strength    = 0.75f;  // stable-diffusion.cpp:3718 (read only with an init latent)
}

// locate libggml-mi355x.so next to this library (the GGML_BACKEND_DL convention:
// "a shared object libggml-<name>.so next to the binary", SURVEY.md §8(b) Discovery)
static std::string self_dir() {
    Dl_info info;
    if (dladdr((void*)&self_dir, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        size_t s      = p.find_last_of('/');
        return s == std::string::npos ? "." : p.substr(0, s);
    }
    return ".";
}

sdm_ctx_t* sdm_new_ctx(const sdm_ctx_params_t* params) { return sdm_new_ctx_variant(params, SDM_UNET_PLAIN); }

sdm_ctx_t* sdm_new_ctx_variant(const sdm_ctx_params_t* params, int variant) {
    if (variant < SDM_UNET_PLAIN || variant > SDM_UNET_PIX2PIX) {
        set_error("sdm_new_ctx_variant: variant must be one of sdm_unet_variant_t");
        return nullptr;
    }
    if (variant != SDM_UNET_PLAIN && params->model != SD_MODEL_SD15 && params->model != SD_MODEL_SDXL && params->model != SD_MODEL_SD15_TINY && params->model != SD_MODEL_SDXL_TINY) {
        set_error("sdm_new_ctx_variant: inpaint / pix2pix variants exist for the UNet families (SD15, SDXL and their tiny forms) only");
        return nullptr;
    }
    const char* dev_name = params->backend ? params->backend : "MI355X0";
    ggml_backend_dev_t dev = ggml_backend_dev_by_name(dev_name);
    if (!dev && !params->backend) {
        // default device: load the product backend plug-in; no CPU fallback exists in the product
        const std::string path = self_dir() + "/libggml-mi355x.so";
        if (!ggml_backend_load(path.c_str())) {
            set_error("MI355X backend plug-in missing or failed to load: " + path);
            return nullptr;
        }
        dev = ggml_backend_dev_by_name(dev_name);
    }
    if (!dev) {
        set_error(std::string("no ggml device named '") + dev_name + "' (is a gfx950 GPU visible?)");
        return nullptr;
    }
    ggml_backend_t backend = ggml_backend_dev_init(dev, nullptr);
    if (!backend) {
        set_error("ggml_backend_dev_init failed");
        return nullptr;
    }
    sdm_ctx_t* ctx = new sdm_ctx_t();
    ctx->params   = *params;
    ctx->backend  = backend;
    ctx->variant  = variant;

    const bool xl   = params->model == SD_MODEL_SDXL || params->model == SD_MODEL_SDXL_TINY;
    const bool tiny = params->model == SD_MODEL_SD15_TINY || params->model == SD_MODEL_SDXL_TINY;
    const bool flux     = params->model == SD_MODEL_FLUX_DEV || params->model == SD_MODEL_FLUX_TINY || params->model == SD_MODEL_FLUX_WIDE1 || params->model == SD_MODEL_FLUX_WIDE8;
    const bool dit      = params->model == SD_MODEL_SD35_LARGE || params->model == SD_MODEL_SD35_TINY || params->model == SD_MODEL_SD35_WIDE2 || params->model == SD_MODEL_SD35_WIDE8 || params->model == SD_MODEL_SD3M_TINY || flux;
    const bool dit_tiny = params->model == SD_MODEL_SD35_TINY || params->model == SD_MODEL_FLUX_TINY || params->model == SD_MODEL_SD3M_TINY;
    UNetConfig ucfg = tiny ? UNetConfig::tiny(xl) : (xl ? UNetConfig::sdxl_base() : UNetConfig::sd15());
    ucfg.in_channels += ctx->concat_channels();  // input_blocks.0.0 alone is wider (model_loader.cpp: ne[2] == 9 inpaint, 8 pix2pix)
    VaeConfig vcfg  = (tiny || dit_tiny) ? VaeConfig::tiny() : (xl ? VaeConfig::sdxl() : VaeConfig::sd15());
    if (tiny && xl) vcfg.scale_factor = 0.13025f;
    if (dit) {  // SD3 VAE: 16 latent channels, no post_quant_conv (auto_encoder_kl.hpp:548-556, 682-684)
        vcfg.z_channels   = 16;
        vcfg.use_quant    = false;
        vcfg.scale_factor = flux ? 0.3611f : 1.5305f;  // auto_encoder_kl.hpp:682-687
        vcfg.shift_factor = flux ? 0.1159f : 0.0609f;
    }

    ctx->unet_runner.backend        = backend;
    ctx->unet_runner.ps.linear_type = (ggml_type)params->wtype;
    ctx->is_dit                     = dit;
    ctx->is_flux                    = flux;
    if (flux) {
        ctx->unet_runner.graph_size = 32768 * 4;  // FLUX_GRAPH_SIZE headroom
        ctx->flux.init(ctx->unet_runner.ps, "model.diffusion_model.", dit_tiny ? FluxConfig::tiny() : (params->model == SD_MODEL_FLUX_WIDE1 ? FluxConfig::flux_wide1() : (params->model == SD_MODEL_FLUX_WIDE8 ? FluxConfig::flux_wide8() : FluxConfig::flux_dev())));
    } else if (dit) {
        ctx->unet_runner.graph_size = 10240 * 8;  // MMDIT_GRAPH_SIZE (mmdit.hpp:14) x our batch headroom
        ctx->mmdit.init(ctx->unet_runner.ps, "model.diffusion_model.", dit_tiny ? (params->model == SD_MODEL_SD3M_TINY ? MMDiTConfig::tiny_medium() : MMDiTConfig::tiny()) : (params->model == SD_MODEL_SD35_WIDE2 ? MMDiTConfig::sd35_wide2() : (params->model == SD_MODEL_SD35_WIDE8 ? MMDiTConfig::sd35_wide8() : MMDiTConfig::sd35_large())));
    } else
        ctx->unet.init(ctx->unet_runner.ps, "model.diffusion_model.", ucfg);  // prefix: stable-diffusion.cpp:1337
    ctx->pair_runner.backend       = backend;
    ctx->pair_runner.graph_size    = 256;
    ctx->skip_runner.backend       = backend;
    ctx->skip_runner.graph_size    = 256;
    ctx->vae_runner.backend        = backend;
    ctx->vae_runner.ps.linear_type = GGML_TYPE_F16;
    ctx->vae_runner.graph_size     = 20480;
    ctx->vae.init(ctx->vae_runner.ps, "first_stage_model.", vcfg);  // prefix: stable-diffusion.cpp:1472
    if (xl) {  // SDXL without an external VAE: Conv2d scale 1/32 on every VAE conv (src/stable-diffusion.cpp:1477-1485)
        ctx->vae_conv2d_scale = 1.f / 32.f;
        ctx->vae.set_conv2d_scale(ctx->vae_conv2d_scale);
    }

    if (!ctx->unet_runner.alloc_weights(params->weight_seed) || !ctx->vae_runner.alloc_weights(params->weight_seed)) {
        set_error("weight buffer allocation failed");
        sdm_free_ctx(ctx);
        return nullptr;
    }
    for (auto* r : {&ctx->unet_runner, &ctx->vae_runner})
        for (auto& sp : r->ps.specs) ctx->all_tensors.push_back({sp.name, sp.tensor});
    ctx->stats.weight_bytes = ggml_backend_buffer_get_size(ctx->unet_runner.weights) + ggml_backend_buffer_get_size(ctx->vae_runner.weights);
    return ctx;
}

void sdm_free_ctx(sdm_ctx_t* ctx) {
    if (!ctx) return;
    ggml_backend_t b = ctx->backend;
    delete ctx;
    ggml_backend_free(b);
}

int64_t sd_tensor_count(sdm_ctx_t* ctx) { return (int64_t)ctx->all_tensors.size(); }
const char* sd_tensor_name(sdm_ctx_t* ctx, int64_t i) { return ctx->all_tensors[i].first.c_str(); }
static ggml_tensor* find_tensor(sdm_ctx_t* ctx, const char* name) {
    for (Runner* r : ctx->runners()) {
        auto it = r->ps.by_name.find(name);
        if (it != r->ps.by_name.end()) return it->second;
    }
    return nullptr;
}
bool sd_tensor_info(sdm_ctx_t* ctx, const char* name, int64_t* ne, int* type, size_t* nbytes) {
    ggml_tensor* t = find_tensor(ctx, name);
    if (!t) return false;
    for (int i = 0; i < 4; ++i) ne[i] = t->ne[i];
    *type   = (int)t->type;
    *nbytes = ggml_nbytes(t);
    return true;
}
bool sd_get_tensor(sdm_ctx_t* ctx, const char* name, void* dst, size_t nbytes) {
    ggml_tensor* t = find_tensor(ctx, name);
    if (!t || nbytes != ggml_nbytes(t)) return false;
    ggml_backend_tensor_get(t, dst, 0, nbytes);
    return true;
}
bool sd_get_tensor_f32(sdm_ctx_t* ctx, const char* name, float* dst, int64_t nelem) {
    ggml_tensor* t = find_tensor(ctx, name);
    if (!t || nelem != ggml_nelements(t)) return false;
    std::vector<uint8_t> raw(ggml_nbytes(t));
    ggml_backend_tensor_get(t, raw.data(), 0, raw.size());
    const int64_t rows = nelem / t->ne[0];
    const size_t rs    = ggml_row_size(t->type, t->ne[0]);
    for (int64_t r = 0; r < rows; ++r) ggml_dequantize_row(t->type, raw.data() + r * rs, dst + r * t->ne[0], t->ne[0]);
    return true;
}
bool sd_set_tensor_f32(sdm_ctx_t* ctx, const char* name, const float* src, int64_t nelem) {
    ggml_tensor* t = find_tensor(ctx, name);
    if (!t || nelem != ggml_nelements(t)) return false;
    std::vector<uint8_t> scratch;
    ctx->unet_runner.upload_f32(t, src, scratch);
    return true;
}

// ---- checkpoint files -> weight buffers ---------------------------------------------
// ModelLoader::load_tensors (src/model_loader.cpp:1180-1260): for every tensor the model declares that the file holds, convert
// file dtype -> f32 -> the parameter's ggml type (convert_tensor, model_loader.cpp:155-205) and ggml_backend_tensor_set it.
// Returns the number of parameters loaded, or -1 on a file / shape error; tensors the file does not name keep their current values.
static bool ensure_text_encoders(sdm_ctx_t* ctx);
static bool ensure_vae_encoder(sdm_ctx_t* ctx);
static bool ensure_tae(sdm_ctx_t* ctx);

static NameDialect name_dialect(const sdm_ctx_t* ctx) {
    NameDialect d;
    d.unet_family = !ctx->is_dit;
    d.flux        = ctx->is_flux;
    if (!ctx->is_dit) {
        const UNetConfig& c = ctx->unet.cfg;
        d.unet_levels       = (int)c.channel_mult.size();
        d.unet_res_blocks   = c.num_res_blocks;
        d.sdxl              = c.sdxl;
        d.unet_attn_levels.clear();
        int ds = 1;
        for (int l = 0; l < d.unet_levels; ++l, ds *= 2)
            if (std::find(c.attention_resolutions.begin(), c.attention_resolutions.end(), ds) != c.attention_resolutions.end()) d.unet_attn_levels.push_back(l);
    }
    d.vae_levels = (int)ctx->vae.cfg.ch_mult.size();
    return d;
}

bool sd_convert_tensor_name(sdm_ctx_t* ctx, const char* name, char* out, size_t out_capacity) {
    const std::string r = canonical_tensor_name(name, name_dialect(ctx));
    if (r.size() + 1 > out_capacity) return false;
    memcpy(out, r.c_str(), r.size() + 1);
    return true;
}

int64_t sd_load_weights(sdm_ctx_t* ctx, const char* path, int64_t* n_missing, int64_t* n_unused) { return sd_load_weights_prefixed(ctx, path, nullptr, n_missing, n_unused); }

// scope: when given, only the parameters it names take part (the others are neither loaded nor counted as missing): sd_load_ip_adapter
static int64_t load_weights_scoped(sdm_ctx_t* ctx, const char* path, const char* prefix, int64_t* n_missing, int64_t* n_unused, const std::map<std::string, ggml_tensor*>* scope);
int64_t sd_load_weights_prefixed(sdm_ctx_t* ctx, const char* path, const char* prefix, int64_t* n_missing, int64_t* n_unused) {
    return load_weights_scoped(ctx, path, prefix, n_missing, n_unused, nullptr);
}
static int64_t load_weights_scoped(sdm_ctx_t* ctx, const char* path, const char* prefix, int64_t* n_missing, int64_t* n_unused, const std::map<std::string, ggml_tensor*>* scope) {
    ModelFile mf;
    if (!read_model_file(path, mf)) {
        set_error(mf.error);
        return -1;
    }
    // file names -> canonical names (init_from_file_and_convert_name, model_loader.cpp); OpenCLIP's fused in_proj rows are split into the
    // q / k / v projections the graph registers: rows [0,E) [E,2E) [2E,3E) of the [3E, E] weight (the reference keeps it fused and
    // chunks the activation instead, ggml_extend.hpp:4074-4081 — the same dot products)
    const NameDialect dialect = name_dialect(ctx);
    std::vector<FileTensor> expanded;
    expanded.reserve(mf.tensors.size());
    bool names_te = false, names_enc = false, names_tae = false;
    for (const FileTensor& t : mf.tensors) {
        FileTensor c = t;
        c.name       = canonical_tensor_name(prefix ? std::string(prefix) + t.name : t.name, dialect);
        names_te     = names_te || c.name.rfind("cond_stage_model.", 0) == 0 || c.name.rfind("text_encoders.", 0) == 0;
        names_enc    = names_enc || c.name.rfind("first_stage_model.encoder.", 0) == 0;
        names_tae    = names_tae || c.name.rfind("tae.decoder.layers.", 0) == 0;
        const std::vector<std::string> qkv = split_in_proj_names(c.name);
        const int outer                    = c.n_dims >= 2 ? 1 : 0;  // the fused dimension: rows of the weight, elements of the bias
        if (!qkv.empty() && c.ne[outer] % 3 == 0 && (outer == 1 || !ggml_is_quantized(c.type))) {
            for (int k = 0; k < 3; ++k) {
                FileTensor part = c;
                part.name       = qkv[k];
                part.ne[outer]  = c.ne[outer] / 3;
                part.nbytes     = c.nbytes / 3;
                part.offset     = c.offset + (uint64_t)k * part.nbytes;
                expanded.push_back(part);
            }
        } else {
            expanded.push_back(c);
        }
    }
    std::map<std::string, const FileTensor*> dir;
    for (auto& t : expanded) dir[t.name] = &t;
    std::map<std::string, std::string> undecodable;  // canonical name -> dtype the readers could not decode
    for (auto& kv : mf.undecodable) undecodable[canonical_tensor_name(prefix ? std::string(prefix) + kv.first : kv.first, dialect)] = kv.second;
    if (names_te && !ensure_text_encoders(ctx)) return -1;  // like the conditioners' tensor_storage_map probes (conditioner.hpp:630-651)
    // a checkpoint that carries the VAE encoder / a taesd file: the modules made on first use are made now, so their tensors are loaded instead of reported unused
    if (names_enc && !ensure_vae_encoder(ctx)) return -1;
    if (names_tae && !ensure_tae(ctx)) return -1;
    FILE* f = fopen(path, "rb");
    if (!f) {
        set_error(std::string("cannot open ") + path);
        return -1;
    }
    int64_t loaded = 0, missing = 0;
    std::vector<uint8_t> raw, conv;
    std::vector<float> f32;
    std::map<std::string, bool> used;
    for (auto& nt : ctx->all_tensors) {
        if (scope && !scope->count(nt.first)) continue;
        auto it = dir.find(nt.first);
        if (it == dir.end()) {
            auto ud = undecodable.find(nt.first);
            if (ud != undecodable.end()) {  // the file HAS this parameter, in a dtype we cannot read: leaving the synthetic weights in place would be silent garbage
                set_error("tensor '" + nt.first + "' is stored as " + ud->second + ", which this build cannot decode");
                fclose(f);
                return -1;
            }
            ++missing;
            continue;
        }
        ggml_tensor* t       = nt.second;
        const int64_t n      = ggml_nelements(t);
        // a fused parameter the file keeps as separate tensors (diffusers DiT q / k / v [/ proj_mlp], name_conversion.hpp: "<name>", "<name>.1",
        // "<name>.2", ...): stack the parts along the output dimension (rows of a weight, elements of a bias)
        if (dir.count(nt.first + ".1")) {
            std::vector<const FileTensor*> parts{it->second};
            for (int k = 1;; ++k) {
                auto pk = dir.find(nt.first + "." + std::to_string(k));
                if (pk == dir.end()) break;
                parts.push_back(pk->second);
            }
            const int64_t inner = ggml_n_dims(t) >= 2 ? t->ne[0] : 1, outer_total = n / inner;
            int64_t outer_sum = 0;
            bool ok = ggml_n_dims(t) <= 2, native_same = true;
            for (const FileTensor* pt : parts) {
                int64_t pn = 1;
                for (int d = 0; d < 4; ++d) pn *= pt->ne[d];
                ok = ok && pn % inner == 0 && (inner == 1 || pt->ne[0] == inner) && pt->n_dims <= 2;
                const uint64_t want = pt->kind != SrcKind::NATIVE ? pt->nbytes : (uint64_t)ggml_row_size(pt->type, pt->ne[0]) * (uint64_t)(pn / pt->ne[0]);
                ok = ok && pt->nbytes == want;
                outer_sum += pn / inner;
                native_same = native_same && pt->kind == SrcKind::NATIVE && pt->type == t->type;
            }
            if (!ok || outer_sum != outer_total) {
                set_error("fused parts do not add up to the shape of " + nt.first);
                fclose(f);
                return -1;
            }
            if (!native_same) f32.assign((size_t)n, 0.f);
            int64_t o0 = 0;  // first output row of the current part
            for (size_t k = 0; k < parts.size(); ++k) {
                const FileTensor& pt = *parts[k];
                int64_t pn = 1;
                for (int d = 0; d < 4; ++d) pn *= pt.ne[d];
                raw.resize(pt.nbytes);
                if (fseek(f, (long)pt.offset, SEEK_SET) != 0 || fread(raw.data(), 1, pt.nbytes, f) != pt.nbytes) {
                    set_error("short read for " + nt.first);
                    fclose(f);
                    return -1;
                }
                if (native_same) {
                    ggml_backend_tensor_set(t, raw.data(), (size_t)o0 * ggml_row_size(t->type, inner), pt.nbytes);
                } else if (pt.kind != SrcKind::NATIVE) {
                    decode_src_kind(pt.kind, raw.data(), pn, f32.data() + o0 * inner);
                } else {
                    const int64_t rows = pn / pt.ne[0];
                    const size_t rs    = ggml_row_size(pt.type, pt.ne[0]);
                    for (int64_t r = 0; r < rows; ++r) ggml_dequantize_row(pt.type, raw.data() + r * rs, f32.data() + o0 * inner + r * pt.ne[0], pt.ne[0]);
                }
                o0 += pn / inner;
                used[nt.first + (k ? "." + std::to_string(k) : std::string())] = true;
            }
            if (!native_same) ctx->unet_runner.upload_f32(t, f32.data(), conv);
            ++loaded;
            continue;
        }
        const FileTensor& ft = *it->second;
        int64_t fn           = 1;
        for (int d = 0; d < 4; ++d) fn *= ft.ne[d];
        // shapes must agree up to trailing 1s; Linear / conv weights additionally dim by dim (torch [out,in,kh,kw] == ggml [kw,kh,in,out]);
        // a [out, in] matrix may fill a 1x1 conv kernel [1,1,in,out] (diffusers stores the VAE attention projections as Linear)
        bool same = fn == n;
        const bool lin_as_conv1x1 = ft.n_dims == 2 && t->ne[0] == 1 && t->ne[1] == 1 && ft.ne[0] == t->ne[2] && ft.ne[1] == t->ne[3];
        for (int d = 0; same && !lin_as_conv1x1 && d < 4; ++d) same = ft.ne[d] == t->ne[d] || (ft.n_dims <= 2 && ggml_n_dims(t) <= 2);
        if (same && !lin_as_conv1x1 && ft.n_dims <= 2 && ggml_n_dims(t) <= 2) same = ft.ne[0] == t->ne[0];
        if (!same) {
            set_error("shape mismatch for " + nt.first);
            fclose(f);
            return -1;
        }
        // the readers validated nbytes against the file's own shape; here against what the copies below will touch
        const uint64_t want = ft.kind != SrcKind::NATIVE ? ft.nbytes : (uint64_t)ggml_row_size(ft.type, ft.ne[0]) * (uint64_t)(n / ft.ne[0]);
        if (ft.nbytes != want || (ft.type == t->type && ft.kind == SrcKind::NATIVE && ft.nbytes != ggml_nbytes(t))) {
            set_error("size mismatch for tensor '" + nt.first + "'");
            fclose(f);
            return -1;
        }
        raw.resize(ft.nbytes);
        if (fseek(f, (long)ft.offset, SEEK_SET) != 0 || fread(raw.data(), 1, ft.nbytes, f) != ft.nbytes) {
            set_error("short read for " + nt.first);
            fclose(f);
            return -1;
        }
        if (ft.kind != SrcKind::NATIVE) {
            f32.resize(n);
            decode_src_kind(ft.kind, raw.data(), n, f32.data());
            ctx->unet_runner.upload_f32(t, f32.data(), conv);
        } else if (ft.type == t->type) {
            ggml_backend_tensor_set(t, raw.data(), 0, ggml_nbytes(t));
        } else {
            f32.resize(n);
            const int64_t rows = n / ft.ne[0];
            const size_t rs    = ggml_row_size(ft.type, ft.ne[0]);
            for (int64_t r = 0; r < rows; ++r) ggml_dequantize_row(ft.type, raw.data() + r * rs, f32.data() + r * ft.ne[0], ft.ne[0]);
            ctx->unet_runner.upload_f32(t, f32.data(), conv);
        }
        used[nt.first] = true;
        ++loaded;
    }
    fclose(f);
    if (n_missing) *n_missing = missing;
    if (n_unused) *n_unused = (int64_t)expanded.size() - (int64_t)used.size();
    // The reference runs SDXL's VAE with Conv2d scale 1/32 only when NO valid external VAE is given (or --force-sdxl-vae-conv-scale is set): a fixed fp16 VAE
    // loaded through --vae keeps scale 1 (src/stable-diffusion.cpp:1477-1485).  Loading a file under the VAE prefix IS the --vae path here, so a
    // successful load of VAE tensors restores scale 1 (round-5 advice); sd_set_vae_conv2d_scale(ctx, 1/32) afterwards is the force flag.
    if (loaded > 0 && prefix && strncmp(prefix, "first_stage_model", 17) == 0 && ctx->vae_conv2d_scale != 1.f) {
        fprintf(stderr, "[sd-mi355x] external VAE loaded: Conv2d scale %.5f -> 1 (call sd_set_vae_conv2d_scale to force a scale)\n", (double)ctx->vae_conv2d_scale);
        ctx->vae_conv2d_scale = 1.f;
        ctx->vae.set_conv2d_scale(1.f);
        if (ctx->vae_enc_ready) ctx->vae_enc.set_conv2d_scale(1.f);
    }
    return loaded;
}

// ---- text encoders + conditioner ----------------------------------------------------
// Which encoders a family owns, their parameter prefixes and output wiring: FrozenCLIPEmbedderWithCustomWords (conditioner.hpp:169-190),
// SD3CLIPEmbedder (:623-652), FluxCLIPEmbedder (:1034-1062).  Weights are synthetic (weight_seed) until sd_load_weights overwrites them.
static bool ensure_text_encoders(sdm_ctx_t* ctx) {
    if (ctx->te) return true;
    std::unique_ptr<sdm_ctx_t::TextEncoders> te(new sdm_ctx_t::TextEncoders());
    const int m     = (int)ctx->params.model;
    const bool tiny = m == SD_MODEL_SD15_TINY || m == SD_MODEL_SDXL_TINY || m == SD_MODEL_SD35_TINY || m == SD_MODEL_FLUX_TINY || m == SD_MODEL_SD3M_TINY;
    ConditionerSpec& sp = te->spec;
    ClipTextConfig lc, gc;
    T5Config tc;
    std::string lp, gp, tp;
    if (m == SD_MODEL_SD15 || m == SD_MODEL_SD15_TINY) {
        sp.family = CondFamily::SD1;
        lc        = tiny ? ClipTextConfig::tiny(64, 4, 0, false, true) : ClipTextConfig::vit_l(true);
        lp        = "cond_stage_model.transformer.text_model.";
    } else if (m == SD_MODEL_SDXL || m == SD_MODEL_SDXL_TINY) {
        sp.family  = CondFamily::SDXL;
        sp.has_g   = true;
        lc         = tiny ? ClipTextConfig::tiny(24, 2, 0, false, false) : ClipTextConfig::vit_l(false);
        gc         = tiny ? ClipTextConfig::tiny(40, 2, 48, true, false) : ClipTextConfig::vit_bigg(false);
        lp         = "cond_stage_model.transformer.text_model.";
        gp         = "cond_stage_model.1.transformer.text_model.";
        sp.adm_dim = ctx->unet.cfg.adm_in_channels;
        sp.ts_dim  = tiny ? 8 : 256;
    } else if (m == SD_MODEL_SD35_LARGE || m == SD_MODEL_SD35_TINY || m == SD_MODEL_SD35_WIDE2 || m == SD_MODEL_SD35_WIDE8 || m == SD_MODEL_SD3M_TINY) {
        sp.family = CondFamily::SD3;
        sp.has_g = sp.has_t5 = true;
        lc = tiny ? ClipTextConfig::tiny(24, 2, 0, false, false) : ClipTextConfig::vit_l(false);
        gc = tiny ? ClipTextConfig::tiny(40, 2, 40, true, false) : ClipTextConfig::vit_bigg(false);
        tc = tiny ? T5Config::tiny(96) : T5Config::xxl();
        lp = "text_encoders.clip_l.transformer.text_model.";
        gp = "text_encoders.clip_g.transformer.text_model.";
        tp = "text_encoders.t5xxl.transformer.";
    } else {
        sp.family   = CondFamily::FLUX;
        sp.has_t5   = true;
        sp.t5_chunk = tiny ? 32 : 256;
        lc          = tiny ? ClipTextConfig::tiny(64, 4, 0, false, true) : ClipTextConfig::vit_l(true);
        tc          = tiny ? T5Config::tiny(96) : T5Config::xxl();
        lp          = "text_encoders.clip_l.transformer.text_model.";
        tp          = "text_encoders.t5xxl.transformer.";
    }
    sp.l_dim  = lc.hidden_size;
    sp.g_dim  = gc.hidden_size;
    sp.g_proj = gc.projection_dim;
    sp.t5_dim = tc.model_dim;
    sp.eos_id = (int32_t)lc.vocab_size - 1;  // 49407 = <|endoftext|> of the 49408-entry CLIP vocabulary
    auto setup = [&](Runner& r, size_t graph_size) {
        r.backend        = ctx->backend;
        r.ps.linear_type = (ggml_type)ctx->params.wtype;
        r.graph_size     = graph_size;
    };
    setup(te->l_runner, 2048);  // clip.hpp:522
    te->clip_l.init(te->l_runner.ps, lp, lc);
    if (sp.has_g) {
        setup(te->g_runner, 4096);
        te->clip_g.init(te->g_runner.ps, gp, gc);
    }
    if (sp.has_t5) {
        setup(te->t5_runner, 4096);
        te->t5.init(te->t5_runner.ps, tp, tc);
    }
    ctx->te = std::move(te);
    for (Runner* r : ctx->runners()) {
        if (r == &ctx->unet_runner || r == &ctx->vae_runner) continue;
        if (!r->alloc_weights(ctx->params.weight_seed)) {
            set_error("text-encoder weight buffer allocation failed");
            ctx->te.reset();
            return false;
        }
    }
    for (Runner* r : ctx->runners()) {
        if (r == &ctx->unet_runner || r == &ctx->vae_runner) continue;
        for (auto& spn : r->ps.specs) ctx->all_tensors.push_back({spn.name, spn.tensor});
        ctx->stats.weight_bytes += ggml_backend_buffer_get_size(r->weights);
    }
    return true;
}

// CLIPTextModelRunner::build_graph / compute (clip.hpp:516-583)
static bool te_clip_forward(sdm_ctx_t* ctx, int which, const int32_t* ids, int64_t n_tokens, size_t max_token_idx, bool return_pooled, int clip_skip, std::vector<float>& out) {
    if (!ensure_text_encoders(ctx)) return false;
    auto& te = *ctx->te;
    if (which < 0 || which > 1 || (which == 1 && !te.spec.has_g)) {
        set_error("this model family has no such CLIP tower");
        return false;
    }
    const ClipTextModel& m = which == 0 ? te.clip_l : te.clip_g;
    const int64_t L        = m.cfg.n_token;
    if (n_tokens <= 0 || n_tokens % L != 0) {  // clip.hpp:509-512: longer inputs fold into a batch of n_token-long rows
        set_error("CLIP input length must be a positive multiple of 77");
        return false;
    }
    const int64_t N = n_tokens / L;
    for (int64_t i = 0; i < n_tokens; ++i)
        if (ids[i] < 0 || ids[i] >= m.cfg.vocab_size) {
            set_error("token id out of range");
            return false;
        }
    if (max_token_idx >= (size_t)n_tokens) {
        set_error("max_token_idx out of range");
        return false;
    }
    const std::vector<float> mask = ClipTextModel::causal_mask((int)L);
    out.resize((size_t)(return_pooled ? (m.text_projection ? m.cfg.projection_dim : m.cfg.hidden_size) : m.cfg.hidden_size * n_tokens));
    auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
        g.flash_attn     = ctx->params.diffusion_flash_attn;
        ggml_tensor* tid = ggml_new_tensor_2d(g.ctx, GGML_TYPE_I32, L, N);
        ggml_set_input(tid);
        in.push_back({tid, ids, ggml_nbytes(tid)});
        ggml_tensor* tm = ggml_new_tensor_2d(g.ctx, GGML_TYPE_F32, L, L);
        ggml_set_input(tm);
        in.push_back({tm, mask.data(), ggml_nbytes(tm)});
        return m.forward(g, tid, tm, max_token_idx, return_pooled, clip_skip);
    };
    return te.runner(which)->compute(build, out.data(), out.size() * sizeof(float));
}

// T5Runner::build_graph / compute (t5.hpp:422-461); no padding mask (SD3 / FLUX pass none)
static bool te_t5_forward(sdm_ctx_t* ctx, const int32_t* ids, int64_t n_tokens, std::vector<float>& out) {
    if (!ensure_text_encoders(ctx)) return false;
    auto& te = *ctx->te;
    if (!te.spec.has_t5) {
        set_error("this model family has no T5 encoder");
        return false;
    }
    const T5Model& m = te.t5;
    if (n_tokens <= 0) {
        set_error("empty T5 input");
        return false;
    }
    for (int64_t i = 0; i < n_tokens; ++i)
        if (ids[i] < 0 || ids[i] >= m.cfg.vocab_size) {
            set_error("token id out of range");
            return false;
        }
    const std::vector<int32_t> buckets = T5Model::relative_position_buckets((int)n_tokens, (int)n_tokens);
    out.resize((size_t)(m.cfg.model_dim * n_tokens));
    auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
        g.flash_attn     = ctx->params.diffusion_flash_attn;
        ggml_tensor* tid = ggml_new_tensor_2d(g.ctx, GGML_TYPE_I32, n_tokens, 1);
        ggml_set_input(tid);
        in.push_back({tid, ids, ggml_nbytes(tid)});
        ggml_tensor* tb = ggml_new_tensor_2d(g.ctx, GGML_TYPE_I32, n_tokens, n_tokens);
        ggml_set_input(tb);
        in.push_back({tb, buckets.data(), ggml_nbytes(tb)});
        return m.forward(g, tid, tb, nullptr);
    };
    return te.t5_runner.compute(build, out.data(), out.size() * sizeof(float));
}

bool sd_text_encoders_init(sdm_ctx_t* ctx) { return ensure_text_encoders(ctx); }

int64_t sd_clip_forward(sdm_ctx_t* ctx, int which, const int32_t* ids, int n_tokens, int max_token_idx, bool return_pooled, int clip_skip, float* out, int64_t out_capacity) {
    std::vector<float> o;
    if (max_token_idx < 0) {
        set_error("max_token_idx out of range");
        return -1;
    }
    if (!te_clip_forward(ctx, which, ids, n_tokens, (size_t)max_token_idx, return_pooled, clip_skip, o)) return -1;
    if ((int64_t)o.size() > out_capacity) {
        set_error("output buffer too small");
        return -1;
    }
    std::copy(o.begin(), o.end(), out);
    return (int64_t)o.size();
}

int64_t sd_t5_forward(sdm_ctx_t* ctx, const int32_t* ids, int n_tokens, float* out, int64_t out_capacity) {
    std::vector<float> o;
    if (!te_t5_forward(ctx, ids, n_tokens, o)) return -1;
    if ((int64_t)o.size() > out_capacity) {
        set_error("output buffer too small");
        return -1;
    }
    std::copy(o.begin(), o.end(), out);
    return (int64_t)o.size();
}

int sd_t5_relative_position_buckets(int q_len, int k_len, int32_t* out) {
    const std::vector<int32_t> b = T5Model::relative_position_buckets(q_len, k_len);
    std::copy(b.begin(), b.end(), out);
    return (int)b.size();
}

bool sd_get_learned_condition(sdm_ctx_t* ctx, const sd_token_list_t* clip_l, const sd_token_list_t* clip_g, const sd_token_list_t* t5, int clip_skip, int width,
                              int height, bool zero_out_masked, float* crossattn_out, int64_t crossattn_capacity, int64_t* crossattn_ne, float* vector_out,
                              int64_t vector_capacity, int64_t* vector_n) {
    if (!ensure_text_encoders(ctx)) return false;
    auto to_list = [](const sd_token_list_t* t) {
        TokenList l;
        if (t && t->n > 0) {
            l.ids.assign(t->ids, t->ids + t->n);
            if (t->weights)
                l.weights.assign(t->weights, t->weights + t->n);
            else
                l.weights.assign((size_t)t->n, 1.0f);
        }
        return l;
    };
    EncoderFns fn;
    fn.clip = [&](int which, const std::vector<int32_t>& ids, size_t max_idx, bool pooled, int skip, std::vector<float>& o) {
        return te_clip_forward(ctx, which, ids.data(), (int64_t)ids.size(), max_idx, pooled, skip, o);
    };
    fn.t5 = [&](const std::vector<int32_t>& ids, std::vector<float>& o) { return te_t5_forward(ctx, ids.data(), (int64_t)ids.size(), o); };
    Condition c;
    std::string err;
    if (!get_learned_condition(ctx->te->spec, fn, to_list(clip_l), to_list(clip_g), to_list(t5), clip_skip, width, height, zero_out_masked, c, err)) {
        if (!err.empty()) set_error(err);
        return false;
    }
    if (crossattn_ne) {
        crossattn_ne[0] = c.ctx_dim;
        crossattn_ne[1] = c.n_tokens;
    }
    if (vector_n) *vector_n = (int64_t)c.vec.size();
    if (crossattn_out) {
        if ((int64_t)c.crossattn.size() > crossattn_capacity) {
            set_error("c_crossattn buffer too small");
            return false;
        }
        std::copy(c.crossattn.begin(), c.crossattn.end(), crossattn_out);
    }
    if (vector_out && !c.vec.empty()) {
        if ((int64_t)c.vec.size() > vector_capacity) {
            set_error("c_vector buffer too small");
            return false;
        }
        std::copy(c.vec.begin(), c.vec.end(), vector_out);
    }
    return true;
}

// ---- one UNet forward ---------------------------------------------------------------------------
// host-built side inputs of one model call (FLUX: guidance vector and rotary table, flux.hpp:1457-1500)
struct ModelSideInputs {
    std::vector<float> guidance;
    const std::vector<float>* pe_table = nullptr;
    const std::vector<float>& pe() const { return *pe_table; }
};
static bool prepare_side_inputs(sdm_ctx_t* ctx, int w, int h, int n, int64_t n_tokens, bool has_y, ModelSideInputs& si) {
    if (!ctx->is_flux) return true;
    if (!has_y) {
        set_error("FLUX needs the pooled text vector y");
        return false;
    }
    si.guidance.assign(n, ctx->guidance);
    // the rotary table depends on the latent size and the text length only: 12 ms of sin/cos per call at 1024x1024 + 256 tokens if rebuilt
    // every forward like the reference does (flux.hpp:1457-1500) — kept per context instead
    if (ctx->pe_cache.empty() || ctx->pe_h != h || ctx->pe_w != w || ctx->pe_tokens != n_tokens) {
        ctx->pe_cache  = gen_flux_pe(h, w, ctx->flux.cfg.patch_size, (int)n_tokens, ctx->flux.cfg.axes_dim, (float)ctx->flux.cfg.theta);
        ctx->pe_h      = h;
        ctx->pe_w      = w;
        ctx->pe_tokens = n_tokens;
    }
    si.pe_table = &ctx->pe_cache;
    return true;
}
// the denoiser network on an existing latent tensor tx [w,h,c,n]: declares the remaining graph inputs and calls the family's forward
static ggml_tensor* build_model_call(sdm_ctx_t* ctx, GraphCtx& g, std::vector<HostInput>& in, ggml_tensor* tx, int n, const float* timesteps, const float* context,
                                     int64_t ctx_dim, int64_t n_tokens, int64_t ctx_n, const float* y, int64_t y_dim, int64_t y_n, const ModelSideInputs& si,
                                     ggml_tensor* c_concat = nullptr, const float* ip_data = nullptr, int64_t n_ip = 0, int ip_n = 0, float ip_scale = 0.f) {
    g.flash_attn    = ctx->params.diffusion_flash_attn;
    g.conv_direct   = ctx->params.diffusion_conv_direct;
    ggml_tensor* tt = ggml_new_tensor_1d(g.ctx, GGML_TYPE_F32, n);
    ggml_set_input(tt);
    in.push_back({tt, timesteps, ggml_nbytes(tt)});
    ggml_tensor* tc = ggml_new_tensor_3d(g.ctx, GGML_TYPE_F32, ctx_dim, n_tokens, ctx_n);
    ggml_set_input(tc);
    in.push_back({tc, context, ggml_nbytes(tc)});
    ggml_tensor* ty = nullptr;
    if (y != nullptr) {
        ty = ggml_new_tensor_2d(g.ctx, GGML_TYPE_F32, y_dim, y_n);
        ggml_set_input(ty);
        in.push_back({ty, y, ggml_nbytes(ty)});
    }
    ggml_tensor* ip_context = nullptr;
    if (ip_data) {  // image tokens [ip_dim, n_ip, ip_n] (UNet families with an initialised adapter; the callers checked)
        ip_context = ggml_new_tensor_3d(g.ctx, GGML_TYPE_F32, ctx->ip_dim, n_ip, ip_n);
        ggml_set_input(ip_context);
        in.push_back({ip_context, ip_data, ggml_nbytes(ip_context)});
    }
    if (ctx->is_flux) {
        // guidance [N] and the rotary table are host-built inputs of every call (flux.hpp:1457-1500: pe_vec generated on the CPU and uploaded)
        ggml_tensor* tg = ggml_new_tensor_1d(g.ctx, GGML_TYPE_F32, n);
        ggml_set_input(tg);
        in.push_back({tg, si.guidance.data(), ggml_nbytes(tg)});
        const FluxConfig& fc = ctx->flux.cfg;
        ggml_tensor* tp      = ggml_new_tensor_4d(g.ctx, GGML_TYPE_F32, 2, 2, fc.hidden_size / fc.num_heads / 2, (int64_t)si.pe().size() / (2 * (fc.hidden_size / fc.num_heads)));
        ggml_set_input(tp);
        in.push_back({tp, si.pe().data(), ggml_nbytes(tp)});
        return ctx->flux.forward(g, tx, tt, tc, ty, tg, tp);
    }
    return ctx->is_dit ? ctx->mmdit.forward(g, tx, tt, tc, ty) : ctx->unet.forward(g, tx, tt, tc, ty, c_concat, ip_context, ip_scale);
}

// skip: the joint blocks a skip-layer-guidance forward leaves out (MMDiT only; NULL / empty = the whole model)
static bool unet_forward_skip(sdm_ctx_t* ctx, const float* x, int w, int h, int c, int n, const float* timesteps, const float* context, int64_t ctx_dim, int64_t n_tokens,
                              int64_t ctx_n, const float* y, int64_t y_dim, int64_t y_n, float* out, const std::vector<int>* skip, const float* c_concat = nullptr,
                              int cc = 0, int concat_n = 0, const float* ip_context = nullptr, int64_t n_ip = 0, int ip_n = 0, float ip_scale = 0.f) {
    Runner& r = ctx->unet_runner;
    if (!ip_context && ctx->ip_call.data) {  // a sampling forward of the host loop with the context's token state
        ip_context = ctx->ip_call.data;
        n_ip       = ctx->ip_set_n;
        ip_n       = ctx->ip_call.ip_n;
        ip_scale   = ctx->ip_strength;
    }
    if (ip_context && ip_scale != 0.f) {
        if (!ctx->ip_ready) {
            set_error("ip_context given, but no IP-Adapter is initialised on this context (sd_ip_adapter_init / sd_load_ip_adapter)");
            return false;
        }
        if (n_ip < 1 || ip_n < 1 || n % ip_n != 0) {
            set_error("ip_context must hold at least one token, and its batch must be 1 or divide the batch of x");
            return false;
        }
    } else {
        ip_context = nullptr;  // block.hpp:382: no tokens or a zero scale emit nothing
    }
    if (ctx->variant != SDM_UNET_PLAIN && !c_concat) {  // never a silent zero-fill of the extra input channels
        set_error("model needs c_concat (an inpaint / pix2pix UNet: sd_unet_forward_concat)");
        return false;
    }
    if (c_concat && (cc != ctx->concat_channels() || cc < 1)) {
        set_error("c_concat has " + std::to_string(cc) + " channels, the model takes " + std::to_string(ctx->concat_channels()));
        return false;
    }
    if (c_concat && (concat_n < 1 || n % concat_n != 0)) {  // (a divisor in between is tiled like 1 is, image i reads row i % concat_n: the host loop's fused branches)
        set_error("c_concat batch must be 1 or the batch of x");
        return false;
    }
    ModelSideInputs si;
    if (!prepare_side_inputs(ctx, w, h, n, n_tokens, y != nullptr, si)) return false;
    if (skip && skip->empty()) skip = nullptr;
    auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
        ggml_tensor* tx = ggml_new_tensor_4d(g.ctx, GGML_TYPE_F32, w, h, c, n);
        ggml_set_input(tx);
        in.push_back({tx, x, ggml_nbytes(tx)});
        ggml_tensor* tcc = nullptr;
        if (c_concat) {
            tcc = ggml_new_tensor_4d(g.ctx, GGML_TYPE_F32, w, h, cc, concat_n);
            ggml_set_input(tcc);
            in.push_back({tcc, c_concat, ggml_nbytes(tcc)});
        }
        g.skip_layers = skip;
        return build_model_call(ctx, g, in, tx, n, timesteps, context, ctx_dim, n_tokens, ctx_n, y, y_dim, y_n, si, tcc, ip_context, n_ip, ip_n, ip_scale);
    };
    char sig[256];
    int so = snprintf(sig, sizeof(sig), "fwd %d %d %d %d %lld %lld %lld %lld %lld %d", w, h, c, n, (long long)ctx_dim, (long long)n_tokens, (long long)ctx_n,
                      (long long)(y ? y_dim : -1), (long long)y_n, (int)ctx->is_flux);
    if (skip)
        for (int l : *skip)
            if (so < (int)sizeof(sig) - 8) so += snprintf(sig + so, sizeof(sig) - so, " s%d", l);
    if (c_concat && so < (int)sizeof(sig) - 24) so += snprintf(sig + so, sizeof(sig) - so, " cc%d n%d", cc, concat_n);
    if (ip_context && so < (int)sizeof(sig) - 48) so += snprintf(sig + so, sizeof(sig) - so, " ip%lld n%d s%a", (long long)n_ip, ip_n, (double)ip_scale);  // the scale is a node parameter
    std::vector<const void*> ptrs{x};
    if (c_concat) ptrs.push_back(c_concat);  // (the order the builder declares its inputs in)
    ptrs.push_back(timesteps);
    ptrs.push_back(context);
    if (y) ptrs.push_back(y);
    if (ip_context) ptrs.push_back(ip_context);
    if (ctx->is_flux) {
        ptrs.push_back(si.guidance.data());
        ptrs.push_back(si.pe().data());
    }
    const bool ok = r.compute(build, out, (size_t)w * h * ctx->out_channels() * n * sizeof(float), sig, ptrs);
    ctx->stats.unet_calls  = r.calls;
    ctx->stats.graph_nodes = r.last_nodes;
    if (r.galloc) ctx->stats.compute_buffer_bytes = ggml_gallocr_get_buffer_size(r.galloc, 0);
    return ok;
}
bool sd_unet_forward(sdm_ctx_t* ctx, const float* x, int w, int h, int c, int n, const float* timesteps, const float* context,
                     int64_t ctx_dim, int64_t n_tokens, int64_t ctx_n, const float* y, int64_t y_dim, int64_t y_n, float* out) {
    return unet_forward_skip(ctx, x, w, h, c, n, timesteps, context, ctx_dim, n_tokens, ctx_n, y, y_dim, y_n, out, nullptr);
}
// the forward of an inpaint / pix2pix UNet: c_concat [w,h,cc,concat_n] is appended to x along the channels in front of input_blocks.0.0 (unet.hpp:554-559)
bool sd_unet_forward_concat(sdm_ctx_t* ctx, const float* x, int w, int h, int c, int n, const float* timesteps, const float* context, int64_t ctx_dim, int64_t n_tokens,
                            int64_t ctx_n, const float* y, int64_t y_dim, int64_t y_n, const float* c_concat, int cc, int concat_n, float* out) {
    if (!c_concat) {
        set_error("sd_unet_forward_concat: c_concat is NULL");
        return false;
    }
    if (ctx->variant == SDM_UNET_PLAIN) {
        set_error("sd_unet_forward_concat: the model takes no c_concat (a plain context)");
        return false;
    }
    return unet_forward_skip(ctx, x, w, h, c, n, timesteps, context, ctx_dim, n_tokens, ctx_n, y, y_dim, y_n, out, nullptr, c_concat, cc, concat_n);
}
// ---- IP-Adapter (src/model/adapter/ip_adapter.hpp, block.hpp:307-393) -----------------------------------------------
// to_k_ip / to_v_ip of every attn2 plus the ImageProjModel, synthetic weights from the seeded initialiser (a file's values are bound afterwards by name like any other parameter)
bool sd_ip_adapter_init(sdm_ctx_t* ctx, int64_t ip_dim, int64_t clip_dim, int64_t num_tokens, uint64_t weight_seed) {
    if (ctx->is_dit) {
        set_error("sd_ip_adapter_init: the IP-Adapter exists for the UNet families (SD15, SDXL and their tiny forms) only");
        return false;
    }
    if (ip_dim < 1 || clip_dim < 1 || num_tokens < 1) {
        set_error("sd_ip_adapter_init: ip_dim, clip_dim and num_tokens must be positive");
        return false;
    }
    if (ctx->ip_ready) {
        if (!ctx->ip_plus && ip_dim == ctx->ip_dim && clip_dim == ctx->ip_clip_dim && num_tokens == ctx->ip_num_tokens) return true;
        set_error("sd_ip_adapter_init: an adapter with other dimensions (ip_dim " + std::to_string(ctx->ip_dim) + ", clip_dim " + std::to_string(ctx->ip_clip_dim) + ", " +
                  std::to_string(ctx->ip_num_tokens) + " tokens) is initialised on this context already");
        return false;
    }
    Runner& r        = ctx->ip_runner;
    r.backend        = ctx->backend;
    r.ps.linear_type = (ggml_type)ctx->params.wtype;
    r.graph_size     = 256;
    ctx->unet.init_ip_adapter(r.ps, ip_dim);
    ctx->ip_proj.init(r.ps, "ip_adapter.image_proj.", clip_dim, ip_dim, num_tokens);
    if (!r.alloc_weights(weight_seed)) {
        ctx->unet.drop_ip_adapter();  // no attn2 may claim projections that have no buffer
        set_error("IP-Adapter weight buffer allocation failed");
        return false;
    }
    for (auto& sp : r.ps.specs) ctx->all_tensors.push_back({sp.name, sp.tensor});
    ctx->stats.weight_bytes += ggml_backend_buffer_get_size(r.weights);
    ctx->ip_dim        = ip_dim;
    ctx->ip_clip_dim   = clip_dim;
    ctx->ip_num_tokens = num_tokens;
    ctx->ip_ready      = true;
    ctx->unet_runner.drop_cache();  // a cached forward graph was built without the adapter's nodes
    return true;
}
// An adapter file ("ip_adapter.<idx>.to_{k,v}_ip.weight", "image_proj.{proj,norm}.*"; names converted by ip_adapter_to_ldm): the dimensions are read from its shapes as
// IPAdapterRunner reads them (ip_adapter.hpp:159-175) — ip_dim = to_k_ip's input width, clip_dim = proj's, num_tokens = proj's rows / norm's width — the adapter is
// initialised from them if it is not yet, and the file's tensors are bound to the adapter's parameters only.  Returns the number loaded, -1 on error.
bool sd_ip_adapter_init_plus(sdm_ctx_t* ctx, int64_t ip_dim, int64_t dim, int64_t depth, int64_t num_queries, int64_t embed_dim, int64_t ff_inner, uint64_t weight_seed);
int64_t sd_load_ip_adapter(sdm_ctx_t* ctx, const char* path, int64_t* n_missing, int64_t* n_unused) {
    if (ctx->is_dit) {
        set_error("sd_load_ip_adapter: the IP-Adapter exists for the UNet families (SD15, SDXL and their tiny forms) only");
        return -1;
    }
    ModelFile mf;
    if (!path || !read_model_file(path, mf)) {
        set_error(path ? mf.error : std::string("sd_load_ip_adapter: NULL path"));
        return -1;
    }
    const NameDialect dialect = name_dialect(ctx);
    int64_t ip_dim = 0, clip_dim = 0, proj_rows = 0, norm_dim = 0;
    // a "plus" file (ip_adapter.hpp:128-158): told by image_proj.latents; the Resampler's shapes as IPAdapterRunner reads them, with its defaults where a tensor is absent
    bool is_plus = false;
    int64_t rs_dim = 1280, rs_queries = 16, rs_embed = 1280, rs_out = 2048, rs_ff = 5120, rs_depth = 0;
    std::map<std::string, bool> plus_q;
    for (const FileTensor& t : mf.tensors) {
        const std::string c = canonical_tensor_name(t.name, dialect);
        const std::string ipp = "ip_adapter.image_proj.";
        if (c.rfind(ipp, 0) != 0) continue;
        const std::string r = c.substr(ipp.size());
        if (r == "latents") is_plus = true, rs_dim = t.ne[0], rs_queries = t.ne[1];
        if (r == "proj_in.weight") rs_embed = t.ne[0];
        if (r == "proj_out.weight") rs_out = t.ne[1];
        if (r == "layers.0.1.1.weight") rs_ff = t.ne[1];
        plus_q[r] = true;
    }
    if (is_plus) {
        while (plus_q.count("layers." + std::to_string(rs_depth) + ".0.to_q.weight")) ++rs_depth;
        if (!sd_ip_adapter_init_plus(ctx, rs_out, rs_dim, rs_depth, rs_queries, rs_embed, rs_ff, ctx->params.weight_seed)) return -1;
        return load_weights_scoped(ctx, path, nullptr, n_missing, n_unused, &ctx->ip_runner.ps.by_name);
    }
    for (const FileTensor& t : mf.tensors) {
        const std::string c = canonical_tensor_name(t.name, dialect);
        const std::string tail = "attn2.to_k_ip.weight";
        if (c.size() > tail.size() && c.compare(c.size() - tail.size(), tail.size(), tail) == 0 && c.rfind("model.diffusion_model.", 0) == 0) ip_dim = t.ne[0];
        if (c == "ip_adapter.image_proj.proj.weight") {
            clip_dim  = t.ne[0];
            proj_rows = t.ne[1];
        }
        if (c == "ip_adapter.image_proj.norm.weight") norm_dim = t.ne[0];
    }
    if (ip_dim < 1 || clip_dim < 1 || norm_dim < 1 || proj_rows % norm_dim != 0) {
        set_error("sd_load_ip_adapter: the file holds no to_k_ip weight of this family's cross-attentions, or neither image_proj.proj / image_proj.norm (a plain adapter) nor image_proj.latents (a plus adapter)");
        return -1;
    }
    if (norm_dim != ip_dim) {
        set_error("sd_load_ip_adapter: image_proj.norm is " + std::to_string(norm_dim) + " wide, to_k_ip reads " + std::to_string(ip_dim));
        return -1;
    }
    if (!sd_ip_adapter_init(ctx, ip_dim, clip_dim, proj_rows / norm_dim, ctx->params.weight_seed)) return -1;
    return load_weights_scoped(ctx, path, nullptr, n_missing, n_unused, &ctx->ip_runner.ps.by_name);
}
bool sd_ip_adapter_info(sdm_ctx_t* ctx, int64_t* ip_dim, int64_t* clip_dim, int64_t* num_tokens) {
    if (!ctx->ip_ready) return false;
    if (ip_dim) *ip_dim = ctx->ip_dim;
    if (clip_dim) *clip_dim = ctx->ip_clip_dim;
    if (num_tokens) *num_tokens = ctx->ip_num_tokens;
    return true;
}
// The general form: embeds [clip_dim, n_tok, n] (n_tok = 1 on a plain adapter, the tower's token count on a plus one) -> image tokens [ip_dim, num_tokens, n]
bool sd_ip_adapter_project_tokens(sdm_ctx_t* ctx, const float* embeds, int64_t n_tok, int n, float* tokens_out) {
    if (!ctx->ip_ready) {
        set_error("sd_ip_adapter_project_tokens: no IP-Adapter is initialised on this context (sd_ip_adapter_init / sd_ip_adapter_init_plus)");
        return false;
    }
    if (!embeds || !tokens_out || n < 1 || n_tok < 1) {
        set_error("sd_ip_adapter_project_tokens: bad arguments");
        return false;
    }
    if (!ctx->ip_plus) {
        if (n_tok != 1) {
            set_error("sd_ip_adapter_project_tokens: a plain adapter (ImageProjModel) takes one embedding per image");
            return false;
        }
        return sd_ip_adapter_project(ctx, embeds, n, tokens_out);
    }
    if (g_graph_capture != 2) {  // the Resampler's feed-forward is GELU_ERF: ask the backend before a graph with it is submitted (a describe-only capture submits none)
        ggml_init_params ip{ggml_tensor_overhead() * 4, nullptr, true};
        ggml_context* pc  = ggml_init(ip);
        ggml_tensor* node = ggml_gelu_erf(pc, ggml_new_tensor_1d(pc, GGML_TYPE_F32, 4));
        const bool ok     = ggml_backend_supports_op(ctx->backend, node);
        ggml_free(pc);
        if (!ok) {
            set_error("sd_ip_adapter_project: the Resampler needs GELU_ERF, which this backend does not support");
            return false;
        }
    }
    auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
        g.flash_attn    = ctx->params.diffusion_flash_attn;
        ggml_tensor* te = ggml_new_tensor_3d(g.ctx, GGML_TYPE_F32, ctx->ip_clip_dim, n_tok, n);
        ggml_set_input(te);
        in.push_back({te, embeds, ggml_nbytes(te)});
        return ctx->ip_resampler.forward(g, te);
    };
    return ctx->ip_runner.compute(build, tokens_out, (size_t)ctx->ip_dim * ctx->ip_num_tokens * n * sizeof(float));
}
// CLIP image embeddings [clip_dim, n] -> image tokens [ip_dim, num_tokens, n]: a small graph of its own on the context's backend
bool sd_ip_adapter_project(sdm_ctx_t* ctx, const float* embeds, int n, float* tokens_out) {
    if (!ctx->ip_ready) {
        set_error("sd_ip_adapter_project: no IP-Adapter is initialised on this context (sd_ip_adapter_init)");
        return false;
    }
    if (!embeds || !tokens_out || n < 1) {
        set_error("sd_ip_adapter_project: bad arguments");
        return false;
    }
    if (ctx->ip_plus) {  // hidden states [embed_dim, n_tok, n] of the initialised tower
        if (!ctx->cv_ready) {
            set_error("sd_ip_adapter_project: a plus adapter takes [embed_dim, n_tok, n] hidden states; without a vision tower on this context their token count is unknown (sd_ip_adapter_project_tokens)");
            return false;
        }
        return sd_ip_adapter_project_tokens(ctx, embeds, ctx->clip_vision.cfg.num_positions(), n, tokens_out);
    }
    auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
        ggml_tensor* te = ggml_new_tensor_2d(g.ctx, GGML_TYPE_F32, ctx->ip_clip_dim, n);
        ggml_set_input(te);
        in.push_back({te, embeds, ggml_nbytes(te)});
        return ctx->ip_proj.forward(g, te);
    };
    return ctx->ip_runner.compute(build, tokens_out, (size_t)ctx->ip_dim * ctx->ip_num_tokens * n * sizeof(float));
}
// Token state of the sampling entries (sdm_generate_image, sd_sample_latents: host loop, fused branches, device-resident sampler, CFG-pair exchange).  tokens /
// uncond_tokens [ip_dim, n_tokens]; tokens NULL clears; uncond_tokens NULL = the projection of an all-zero embedding (stable-diffusion.cpp:2206-2207 — not zero when
// the projection's LayerNorm has a bias), which has the projection's own token count
bool sd_set_ip_adapter(sdm_ctx_t* ctx, const float* tokens, const float* uncond_tokens, int64_t n_tokens, float strength) {
    if (!tokens) {
        ctx->ip_tokens.clear();
        ctx->ip_uncond.clear();
        ctx->ip_set_n    = 0;
        ctx->ip_strength = 0.f;
        return true;
    }
    if (!ctx->ip_ready) {
        set_error("sd_set_ip_adapter: no IP-Adapter is initialised on this context (sd_ip_adapter_init / sd_load_ip_adapter)");
        return false;
    }
    if (n_tokens < 1 || std::isnan(strength)) {
        set_error("sd_set_ip_adapter: n_tokens must be positive and the strength a number");
        return false;
    }
    const size_t cnt = (size_t)ctx->ip_dim * (size_t)n_tokens;
    std::vector<float> un(cnt);
    if (uncond_tokens) {
        std::copy(uncond_tokens, uncond_tokens + cnt, un.begin());
    } else {
        if (n_tokens != ctx->ip_num_tokens) {
            set_error("sd_set_ip_adapter: the default uncond tokens are the projection of zeros, " + std::to_string(ctx->ip_num_tokens) + " tokens; with " + std::to_string(n_tokens) +
                      " cond tokens uncond_tokens must be given");
            return false;
        }
        const int64_t zt = ctx->ip_plus ? (ctx->cv_ready ? ctx->clip_vision.cfg.num_positions() : 0) : 1;
        if (zt < 1) {
            set_error("sd_set_ip_adapter: the default uncond tokens of a plus adapter are the Resampler's output for all-zero hidden states of the tower's shape; without a vision tower uncond_tokens must be given");
            return false;
        }
        const std::vector<float> zero((size_t)(ctx->ip_clip_dim * zt), 0.f);
        if (!sd_ip_adapter_project_tokens(ctx, zero.data(), zt, 1, un.data())) return false;
    }
    ctx->ip_tokens.assign(tokens, tokens + cnt);
    ctx->ip_uncond   = std::move(un);
    ctx->ip_set_n    = n_tokens;
    ctx->ip_strength = strength;
    return true;
}
// project + set, as the reference does with the CLIP image embedding (stable-diffusion.cpp:2187-2215); embeds [clip_dim]
bool sd_set_ip_adapter_embeds(sdm_ctx_t* ctx, const float* embeds, float strength) {
    if (!embeds) return sd_set_ip_adapter(ctx, nullptr, nullptr, 0, 0.f);
    if (!ctx->ip_ready) {
        set_error("sd_set_ip_adapter_embeds: no IP-Adapter is initialised on this context (sd_ip_adapter_init / sd_load_ip_adapter)");
        return false;
    }
    if (ctx->ip_plus) {
        set_error("sd_set_ip_adapter_embeds: a plus adapter projects hidden states, not one embedding (sd_set_ip_adapter_image, or sd_ip_adapter_project_tokens + sd_set_ip_adapter)");
        return false;
    }
    std::vector<float> tok((size_t)ctx->ip_dim * (size_t)ctx->ip_num_tokens);
    if (!sd_ip_adapter_project(ctx, embeds, 1, tok.data())) return false;
    return sd_set_ip_adapter(ctx, tok.data(), nullptr, ctx->ip_num_tokens, strength);
}
// sd_unet_forward_concat's argument list (c_concat may be NULL on a plain context) plus the image tokens ip_context [ip_dim, n_ip, ip_n] and their scale
bool sd_unet_forward_ip(sdm_ctx_t* ctx, const float* x, int w, int h, int c, int n, const float* timesteps, const float* context, int64_t ctx_dim, int64_t n_tokens,
                        int64_t ctx_n, const float* y, int64_t y_dim, int64_t y_n, const float* c_concat, int cc, int concat_n, const float* ip_context, int64_t n_ip,
                        int ip_n, float ip_scale, float* out) {
    if (ctx->is_dit) {
        set_error("sd_unet_forward_ip: the IP-Adapter exists for the UNet families only");
        return false;
    }
    if (ip_context && !ctx->ip_ready) {
        set_error("sd_unet_forward_ip: no IP-Adapter is initialised on this context (sd_ip_adapter_init)");
        return false;
    }
    if (c_concat && ctx->variant == SDM_UNET_PLAIN) {
        set_error("sd_unet_forward_ip: the model takes no c_concat (a plain context)");
        return false;
    }
    return unet_forward_skip(ctx, x, w, h, c, n, timesteps, context, ctx_dim, n_tokens, ctx_n, y, y_dim, y_n, out, nullptr, c_concat, cc, concat_n, ip_context, n_ip, ip_n, ip_scale);
}
// ---- the "plus" adapters: Resampler (ip_adapter.hpp:34-113) in place of the ImageProjModel ------------------------------------------------
bool sd_ip_adapter_init_plus(sdm_ctx_t* ctx, int64_t ip_dim, int64_t dim, int64_t depth, int64_t num_queries, int64_t embed_dim, int64_t ff_inner, uint64_t weight_seed) {
    if (ctx->is_dit) {
        set_error("sd_ip_adapter_init_plus: the IP-Adapter exists for the UNet families (SD15, SDXL and their tiny forms) only");
        return false;
    }
    if (ip_dim < 1 || dim < 64 || dim % 64 != 0 || depth < 1 || num_queries < 1 || embed_dim < 1 || ff_inner < 1) {
        set_error("sd_ip_adapter_init_plus: every dimension must be positive and dim a multiple of the head size 64");
        return false;
    }
    if (ctx->ip_ready) {
        const Resampler& r = ctx->ip_resampler;
        if (ctx->ip_plus && ip_dim == ctx->ip_dim && dim == r.dim && depth == r.depth && num_queries == r.num_queries && embed_dim == r.embed_dim && ff_inner == r.ff_inner) return true;
        set_error("sd_ip_adapter_init_plus: another adapter (ip_dim " + std::to_string(ctx->ip_dim) + ", " + (ctx->ip_plus ? "plus" : "plain") + ") is initialised on this context already");
        return false;
    }
    Runner& r        = ctx->ip_runner;
    r.backend        = ctx->backend;
    r.ps.linear_type = (ggml_type)ctx->params.wtype;
    r.graph_size     = 1024;  // IPAdapterRunner::build_graph, ip_adapter.hpp:191
    ctx->unet.init_ip_adapter(r.ps, ip_dim);
    ctx->ip_resampler.init(r.ps, "ip_adapter.image_proj.", dim, depth, num_queries, embed_dim, ip_dim, ff_inner);
    if (!r.alloc_weights(weight_seed)) {
        ctx->unet.drop_ip_adapter();
        set_error("IP-Adapter weight buffer allocation failed");
        return false;
    }
    for (auto& sp : r.ps.specs) ctx->all_tensors.push_back({sp.name, sp.tensor});
    ctx->stats.weight_bytes += ggml_backend_buffer_get_size(r.weights);
    ctx->ip_dim        = ip_dim;
    ctx->ip_clip_dim   = embed_dim;
    ctx->ip_num_tokens = num_queries;
    ctx->ip_plus       = true;
    ctx->ip_ready      = true;
    ctx->unet_runner.drop_cache();
    return true;
}
bool sd_ip_adapter_info_ex(sdm_ctx_t* ctx, int64_t* ip_dim, int64_t* clip_dim, int64_t* num_tokens, bool* is_plus) {
    if (!sd_ip_adapter_info(ctx, ip_dim, clip_dim, num_tokens)) return false;
    if (is_plus) *is_plus = ctx->ip_plus;
    return true;
}

// ---- CLIP vision tower (clip.hpp:183-238, 332-464; FrozenCLIPVisionEmbedder, conditioner.hpp:561-613) ------------------------------------
static bool clip_vision_init_cfg(sdm_ctx_t* ctx, const ClipVisionConfig& c, uint64_t weight_seed) {
    if (c.hidden_size < 1 || c.n_head < 1 || c.hidden_size % c.n_head != 0 || c.n_layer < 1 || c.patch_size < 1 || c.image_size < c.patch_size || c.image_size % c.patch_size != 0 ||
        c.projection_dim < 1) {
        set_error("sd_clip_vision_init: hidden must be a positive multiple of heads, layers and projection positive, image_size a positive multiple of patch_size");
        return false;
    }
    if (ctx->cv_ready) {
        const ClipVisionConfig& o = ctx->clip_vision.cfg;
        if (o.hidden_size == c.hidden_size && o.intermediate_size == c.intermediate_size && o.n_head == c.n_head && o.n_layer == c.n_layer && o.image_size == c.image_size &&
            o.patch_size == c.patch_size && o.projection_dim == c.projection_dim)
            return true;
        set_error("sd_clip_vision_init: a vision tower of another shape is initialised on this context already");
        return false;
    }
    Runner& r        = ctx->cv_runner;
    r.backend        = ctx->backend;
    r.ps.linear_type = (ggml_type)ctx->params.wtype;
    r.graph_size     = 4096;
    ctx->clip_vision.init(r.ps, "clip_vision.", c);
    if (!r.alloc_weights(weight_seed)) {
        set_error("CLIP vision tower weight buffer allocation failed");
        return false;
    }
    for (auto& sp : r.ps.specs) ctx->all_tensors.push_back({sp.name, sp.tensor});
    ctx->stats.weight_bytes += ggml_backend_buffer_get_size(r.weights);
    ctx->cv_ready = true;
    return true;
}
bool sd_clip_vision_init(sdm_ctx_t* ctx, int version, const sd_clip_vision_tiny_t* tiny, uint64_t weight_seed) {
    ClipVisionConfig c;
    if (tiny) {
        c = ClipVisionConfig::tiny(tiny->hidden_size, tiny->n_head, tiny->n_layer, tiny->image_size, tiny->patch_size, tiny->projection_dim);
    } else if (version == CLIP_VIT_L_14) {
        c = ClipVisionConfig::vit_l();
    } else if (version == CLIP_VIT_H_14) {
        c = ClipVisionConfig::vit_h();
    } else if (version == CLIP_VIT_BIGG_14) {
        c = ClipVisionConfig::vit_bigg();
    } else {
        set_error("sd_clip_vision_init: version is 0 (ViT-L/14), 1 (ViT-H/14) or 2 (ViT-bigG/14), or a tiny configuration is given");
        return false;
    }
    return clip_vision_init_cfg(ctx, c, weight_seed);
}
bool sd_clip_vision_info(sdm_ctx_t* ctx, sd_clip_vision_info_t* out) {
    if (!ctx->cv_ready || !out) return false;
    const ClipVisionConfig& c = ctx->clip_vision.cfg;
    out->image_size = c.image_size, out->patch_size = c.patch_size, out->hidden_size = c.hidden_size, out->intermediate_size = c.intermediate_size, out->n_head = c.n_head;
    out->n_layer = c.n_layer, out->projection_dim = c.projection_dim, out->num_positions = c.num_positions(), out->use_gelu = c.use_gelu ? 1 : 0;
    return true;
}
// A tower file (HF CLIPVisionModelWithProjection names): loaded under the "clip_vision." prefix with the reference's rule (name_conversion.cpp:1473: the prefix becomes
// the cond-stage tower's, whose conversion leaves the HF vision tree alone but for "vision_model.visual_projection.weight" -> "visual_projection.weight").  The version is
// read off the file's shapes: hidden from the class embedding, layers counted, intermediate from fc1, projection from visual_projection, patch and image size from the
// patch weight and the position table; heads are 16 on every full-size tower, hidden / 64 otherwise.
int64_t sd_load_clip_vision(sdm_ctx_t* ctx, const char* path, int64_t* n_missing, int64_t* n_unused) {
    ModelFile mf;
    if (!path || !read_model_file(path, mf)) {
        set_error(path ? mf.error : std::string("sd_load_clip_vision: NULL path"));
        return -1;
    }
    const NameDialect dialect = name_dialect(ctx);
    const std::string vm      = "clip_vision.vision_model.";
    int64_t hidden = 0, inter = 0, proj = 0, patch = 0, positions = 0, layers = 0;
    std::map<std::string, bool> seen;
    for (const FileTensor& t : mf.tensors) {
        const std::string c = canonical_tensor_name("clip_vision." + t.name, dialect);
        seen[c]             = true;
        if (c == vm + "embeddings.class_embedding") hidden = t.ne[0];
        if (c == vm + "embeddings.patch_embedding.weight") patch = t.ne[0];
        if (c == vm + "embeddings.position_embedding.weight") positions = t.ne[1];
        if (c == vm + "encoder.layers.0.mlp.fc1.weight") inter = t.ne[1];
        if (c == "clip_vision.visual_projection.weight") proj = t.ne[1];
    }
    while (seen.count(vm + "encoder.layers." + std::to_string(layers) + ".layer_norm1.weight")) ++layers;
    int64_t grid = 0;
    while ((grid + 1) * (grid + 1) + 1 <= positions) ++grid;
    if (hidden < 1 || inter < 1 || proj < 1 || patch < 1 || layers < 1 || grid < 1 || grid * grid + 1 != positions) {
        set_error("sd_load_clip_vision: the file is no CLIP vision tower with projection (class_embedding, patch_embedding, position_embedding, encoder layers, visual_projection)");
        return -1;
    }
    ClipVisionConfig c;
    c.hidden_size = hidden, c.intermediate_size = inter, c.n_layer = layers, c.projection_dim = proj, c.patch_size = patch, c.image_size = grid * patch;
    c.n_head   = (hidden == 1024 || hidden == 1280 || hidden == 1664) ? 16 : std::max<int64_t>(hidden / 64, 1);
    c.version  = hidden == 1280 ? CLIP_VIT_H_14 : (hidden == 1664 ? CLIP_VIT_BIGG_14 : CLIP_VIT_L_14);
    c.use_gelu = ClipVisionConfig::gelu_rule(hidden);
    if (!clip_vision_init_cfg(ctx, c, ctx->params.weight_seed)) return -1;
    return load_weights_scoped(ctx, path, "clip_vision.", n_missing, n_unused, &ctx->cv_runner.ps.by_name);
}
// n u8 HWC RGB pictures [n][h][w][3] -> pixel values [S, S, 3, n], S = the tower's image size: the kernel on a backend that exports it, the host restatement on others
static bool clip_preprocess_size(sdm_ctx_t* ctx, const uint8_t* images, int w, int h, int n, int S, float* out) {
    if (!images || !out || w < 1 || h < 1 || n < 1 || S < 1) {
        set_error("sd_clip_preprocess: bad arguments");
        return false;
    }
    std::vector<int32_t> xi, yi;
    clip_preprocess_tables(w, h, S, xi, yi);
    typedef bool (*pre_fn)(ggml_backend_t, const uint8_t*, int, int, int64_t, int, const int*, const int*, float*);
    ggml_backend_dev_t dev = ggml_backend_get_device(ctx->backend);
    ggml_backend_reg_t reg = dev ? ggml_backend_dev_backend_reg(dev) : nullptr;
    pre_fn k               = reg ? (pre_fn)ggml_backend_reg_get_proc_address(reg, "ggml_backend_mi355x_clip_preprocess") : nullptr;
    if (k) {
        if (!k(ctx->backend, images, w, h, n, S, xi.data(), yi.data(), out)) {
            set_error("sd_clip_preprocess: the preprocessing pass could not be run");
            return false;
        }
        return true;
    }
    if (reg && strcmp(ggml_backend_reg_name(reg), "MI355X") == 0) {  // never a quiet fall-back on the product backend
        set_error("sd_clip_preprocess: the MI355X backend does not export ggml_backend_mi355x_clip_preprocess");
        return false;
    }
    clip_preprocess_host(images, w, h, n, S, xi, yi, out);
    return true;
}
bool sd_clip_preprocess_size(sdm_ctx_t* ctx, const uint8_t* images, int w, int h, int n, int size, float* out) { return clip_preprocess_size(ctx, images, w, h, n, size, out); }
bool sd_clip_preprocess(sdm_ctx_t* ctx, const uint8_t* images, int w, int h, int n, float* out) {
    if (!ctx->cv_ready) {
        set_error("sd_clip_preprocess: no vision tower is initialised on this context (sd_clip_vision_init / sd_load_clip_vision); sd_clip_preprocess_size takes the size itself");
        return false;
    }
    return clip_preprocess_size(ctx, images, w, h, n, (int)ctx->clip_vision.cfg.image_size, out);
}
// pixel_values [S, S, 3, n] -> pooled [projection_dim, n], or the hidden state before post_layernorm [hidden, num_positions, n] (clip_skip as CLIPEncoder reads it)
bool sd_clip_vision_encode(sdm_ctx_t* ctx, const float* pixel_values, int n, bool return_pooled, int clip_skip, float* out) {
    if (!ctx->cv_ready) {
        set_error("sd_clip_vision_encode: no vision tower is initialised on this context (sd_clip_vision_init / sd_load_clip_vision)");
        return false;
    }
    const ClipVisionConfig& c = ctx->clip_vision.cfg;
    if (!pixel_values || !out || n < 1) {
        set_error("sd_clip_vision_encode: bad arguments");
        return false;
    }
    auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
        g.flash_attn    = ctx->params.diffusion_flash_attn;
        g.conv_direct   = ctx->params.diffusion_conv_direct;
        ggml_tensor* px = ggml_new_tensor_4d(g.ctx, GGML_TYPE_F32, c.image_size, c.image_size, c.num_channels, n);
        ggml_set_input(px);
        in.push_back({px, pixel_values, ggml_nbytes(px)});
        return ctx->clip_vision.forward(g, px, return_pooled, clip_skip);
    };
    const size_t cnt = (size_t)(return_pooled ? c.projection_dim : c.hidden_size * c.num_positions()) * (size_t)n;
    return ctx->cv_runner.compute(build, out, cnt * sizeof(float));
}
// compute_ip_adapter_tokens (stable-diffusion.cpp:2187-2215): preprocess, encode (pooled; the penultimate hidden state for a plus adapter), project; the uncond tokens
// are the projection of an all-zero embedding of the same shape
bool sd_set_ip_adapter_image(sdm_ctx_t* ctx, const uint8_t* image, int w, int h, float strength) {
    if (!image) return sd_set_ip_adapter(ctx, nullptr, nullptr, 0, 0.f);
    if (!ctx->ip_ready) {
        set_error("sd_set_ip_adapter_image: no IP-Adapter is initialised on this context (sd_ip_adapter_init / _init_plus / sd_load_ip_adapter)");
        return false;
    }
    if (!ctx->cv_ready) {
        set_error("sd_set_ip_adapter_image: no vision tower is initialised on this context (sd_clip_vision_init / sd_load_clip_vision)");
        return false;
    }
    const ClipVisionConfig& c = ctx->clip_vision.cfg;
    const int64_t width       = ctx->ip_plus ? c.hidden_size : c.projection_dim;
    if (width != ctx->ip_clip_dim) {
        set_error("sd_set_ip_adapter_image: the tower hands the adapter " + std::to_string(width) + (ctx->ip_plus ? "-wide hidden states" : "-wide embeddings") + ", the adapter expects " +
                  std::to_string(ctx->ip_clip_dim));
        return false;
    }
    std::vector<float> px((size_t)(c.image_size * c.image_size * 3));
    if (!sd_clip_preprocess(ctx, image, w, h, 1, px.data())) return false;
    const int64_t n_tok = ctx->ip_plus ? c.num_positions() : 1;
    std::vector<float> embed((size_t)(width * n_tok));
    if (!sd_clip_vision_encode(ctx, px.data(), 1, !ctx->ip_plus, ctx->ip_plus ? 2 : -1, embed.data())) return false;
    const size_t cnt = (size_t)ctx->ip_dim * (size_t)ctx->ip_num_tokens;
    std::vector<float> tok(cnt), un(cnt);
    if (!sd_ip_adapter_project_tokens(ctx, embed.data(), n_tok, 1, tok.data())) return false;
    std::fill(embed.begin(), embed.end(), 0.f);
    if (!sd_ip_adapter_project_tokens(ctx, embed.data(), n_tok, 1, un.data())) return false;
    return sd_set_ip_adapter(ctx, tok.data(), un.data(), ctx->ip_num_tokens, strength);
}
int sd_unet_variant(sdm_ctx_t* ctx) { return ctx->variant; }
int sd_concat_channels(sdm_ctx_t* ctx) { return ctx->concat_channels(); }

// the same forward without the listed MMDiT joint blocks (MMDiT::forward's skip_layers, mmdit.hpp:854-866): what skip-layer guidance evaluates
bool sd_unet_forward_skip_layers(sdm_ctx_t* ctx, const float* x, int w, int h, int c, int n, const float* timesteps, const float* context, int64_t ctx_dim, int64_t n_tokens,
                                 int64_t ctx_n, const float* y, int64_t y_dim, int64_t y_n, const int* skip_layers, int n_skip, float* out) {
    if (!ctx->is_dit || ctx->is_flux) {
        set_error("sd_unet_forward_skip_layers: skip layers exist for the MMDiT family only");
        return false;
    }
    const std::vector<int> skip(skip_layers, skip_layers + (n_skip > 0 ? n_skip : 0));
    return unet_forward_skip(ctx, x, w, h, c, n, timesteps, context, ctx_dim, n_tokens, ctx_n, y, y_dim, y_n, out, &skip);
}

// ---- VAE tiling -----------------------------------------------------------------------------------
// The reference's `--vae-tiling` (sd_tiling_params_t): tile sizes VAE::get_tile_sizes (src/model/vae/vae.hpp:89-116), tile counts and the achieved overlap
// sd_tiling_calc_tiles (src/core/ggml_extend.hpp:691-739, non-circular branch), order / positions / the shifted last tile process_tiles_2d (:823-951), the
// blend sd_tensor_merge_2d (:771-821).  Restated here; what differs is WHERE things run: the reference computes one graph per tile and merges on the host,
// this driver stacks tile_batch tiles along the batch dimension of one graph and blends on the device into a canvas that is read back once.
static const int TILE_BATCH_DEFAULT = 16;  // the smallest batch within 3 % of the best time at a 256^2 latent (profiles/vae_tiling_probe.txt; DESIGN.md 1, row "VAE tiling")
static const int TILE_BATCH_MAX     = 32;  // the fused merge kernel's descriptor table (kernels.h: TILE_MERGE_MAX)

struct TileAxis {
    int tile = 0, overlap = 0;             // latent cells
    std::vector<std::pair<int, int>> pos;  // (start, skipped leading cells) per tile
};
// one axis: `requested` cells per tile over `small` cells with `target` overlap
static void tiling_axis(int small, int requested, float target, TileAxis& ax) {
    const int want    = (int)(requested * target);
    const int stride0 = requested - want;
    int count         = (small - want) / stride0;
    const int over    = ((count + 1) * stride0 + want) % small;
    if (over != stride0 && over <= count * (requested / 2 - want)) ++count;  // room for one more tile without passing an overlap of 0.5
    float factor = (float)(requested * count - small) / (float)(requested * (count - 1));
    if (count <= 2) {
        if (small <= requested) {
            count  = 1;
            factor = 0.f;
        } else {
            count  = 2;
            factor = (2 * requested - small) / (float)requested;
        }
    }
    ax.overlap     = (int)(requested * factor);
    ax.tile        = std::min(requested, small);
    const int step = std::max(1, requested - ax.overlap);
    ax.pos.clear();
    bool last = false;
    for (int x = 0; x < small && !last; x += step) {
        int at = x, skip = 0;
        if (x + ax.tile >= small) {  // the last tile ends at the border; what it repeats of its neighbour is skipped by the merge
            at   = small - ax.tile;
            skip = x - at;
            last = true;
        }
        ax.pos.push_back({at, skip});
    }
}
static int tiling_tile_size(int requested, float rel, int64_t latent, float overlap, float encode_factor) {
    int size = 32;
    if (rel > 0.f) {
        if (rel > 1.0) rel = 1 / (rel - rel * overlap + overlap);  // a tile COUNT across the axis
        size = (int)std::round(latent * rel);
    } else if (requested >= 4) {
        size = requested;
    }
    size = (int)(size * encode_factor);
    return std::max(std::min(size, (int)latent), 4);
}
struct TilePlan {
    TileAxis ax, ay;
    int count() const { return (int)(ax.pos.size() * ay.pos.size()); }
};
static bool tiling_plan(int small_w, int small_h, const sdm_tiling_params_t& tp, float encode_factor, TilePlan& pl) {
    if (small_w < 1 || small_h < 1 || !(encode_factor > 0.f)) return false;
    const float target = std::max(std::min(tp.target_overlap, 0.5f), 0.0f);
    tiling_axis(small_w, tiling_tile_size(tp.tile_size_x, tp.rel_size_x, small_w, target, encode_factor), target, pl.ax);
    tiling_axis(small_h, tiling_tile_size(tp.tile_size_y, tp.rel_size_y, small_h, target, encode_factor), target, pl.ay);
    return true;
}
static inline float tile_ramp(float t) { return t * t * t * (t * (6.0f * t - 15.0f) + 10.0f); }
// s(min(rise, fall, 1)) for every cell of one tile along one axis, in OUTPUT cells: start / skip / overlap / tile already scaled, `full` = the canvas extent
static void tile_ramp_vector(float* w, int tile, int start, int skip, int overlap, int full) {
    for (int i = 0; i < tile; ++i) {
        if (i < skip) {
            w[i] = 0.f;  // never read: the merge starts behind the skip
            continue;
        }
        const float rise = (overlap > 0 && start > 0) ? (i - skip) / float(overlap) : 1.f;
        const float fall = (overlap > 0 && start < full - tile) ? (tile - i) / float(overlap) : 1.f;
        w[i]             = tile_ramp(std::min(std::min(rise, fall), 1.f));
    }
}

// dir 0, decode: in = VAE latents [iw, ih, ic, n] -> out [8 iw, 8 ih, 3, n] (the raw decoder output); dir 1, encode: in = pixels in [-1, 1] [iw, ih, 3, n] ->
// moments [iw/8, ih/8, 2 zc, n]; dir 2 (sd_tiling_blend): the identity in place of the model, [iw, ih, ic, n] -> the same shape
static bool vae_tiled(sdm_ctx_t* ctx, int dir, const float* in, int iw, int ih, int ic, int n, float* out) {
    const bool decode = dir == 0;
    const int scale = dir == 2 ? 1 : 8;
    const int sw = decode ? iw : iw / scale, sh = decode ? ih : ih / scale;
    const int oc = decode ? 3 : dir == 2 ? ic : 2 * (int)ctx->vae.cfg.z_channels;
    const sdm_tiling_params_t& tp = ctx->tiling;
    TilePlan pl;
    if (!tiling_plan(sw, sh, tp, dir == 1 ? 2.0f : 1.0f, pl)) {
        set_error("VAE tiling: empty input");
        return false;
    }
    const int T  = pl.count(), ntx = (int)pl.ax.pos.size();
    const int k  = std::max(1, std::min(std::min(tp.tile_batch > 0 ? tp.tile_batch : TILE_BATCH_DEFAULT, TILE_BATCH_MAX), T));
    const int kl = T % k;  // tiles of the short last batch
    // in-tile / out-tile extents and the merge geometry in OUTPUT cells (pixels for decode, latent cells for encode)
    const int itw = pl.ax.tile * (decode ? 1 : scale), ith = pl.ay.tile * (decode ? 1 : scale);
    const int om  = decode ? scale : 1;
    const int otw = pl.ax.tile * om, oth = pl.ay.tile * om, ow = sw * om, oh = sh * om, ovx = pl.ax.overlap * om, ovy = pl.ay.overlap * om;
    const bool blend = ovx > 0 || ovy > 0;  // sd_tensor_merge_2d accumulates when either overlap is positive and stores otherwise

    char key[256];
    snprintf(key, sizeof(key), "%d %d %d %d %d %d | %d %d %d %d | %d %d", dir, iw, ih, ic, n, k, pl.ax.tile, pl.ay.tile, pl.ax.overlap, pl.ay.overlap, ntx, T);
    std::unique_ptr<sdm_ctx_t::TileState>& sp = ctx->tstate[dir];
    if (!sp || sp->key != key) {
        sp.reset(new sdm_ctx_t::TileState());
        auto& st = *sp;
        ggml_init_params ip{0, nullptr, true};
        st.sctx   = ggml_init(ip);
        st.canvas = ggml_new_tensor_4d(st.sctx, GGML_TYPE_F32, ow, oh, oc, n);
        ggml_set_name(st.canvas, "vae_tiling.canvas");
        if (T >= k) st.store[0] = ggml_new_tensor_4d(st.sctx, GGML_TYPE_F32, otw, oth, oc, (int64_t)n * k);
        if (kl > 0) st.store[1] = ggml_new_tensor_4d(st.sctx, GGML_TYPE_F32, otw, oth, oc, (int64_t)n * kl);
        st.wx = ggml_new_tensor_4d(st.sctx, GGML_TYPE_F32, otw, 1, 1, T);
        st.wy = ggml_new_tensor_4d(st.sctx, GGML_TYPE_F32, 1, oth, 1, T);
        st.buf = ggml_backend_alloc_ctx_tensors(st.sctx, ctx->backend);
        if (!st.buf) {
            sp.reset();
            set_error("VAE tiling: canvas allocation failed");
            return false;
        }
        // the ramps depend on the plan alone: computed on the host in f32 and uploaded once per state
        std::vector<float> wx((size_t)otw * T), wy((size_t)oth * T);
        for (int t = 0; t < T; ++t) {
            const auto& px = pl.ax.pos[t % ntx];
            const auto& py = pl.ay.pos[t / ntx];
            tile_ramp_vector(&wx[(size_t)t * otw], otw, px.first * om, px.second * om, ovx, ow);
            tile_ramp_vector(&wy[(size_t)t * oth], oth, py.first * om, py.second * om, ovy, oh);
        }
        ggml_backend_tensor_set(st.wx, wx.data(), 0, wx.size() * sizeof(float));
        ggml_backend_tensor_set(st.wy, wy.data(), 0, wy.size() * sizeof(float));
        st.merge_galloc = ggml_gallocr_new(ggml_backend_get_default_buffer_type(ctx->backend));
        st.key          = key;
        static std::atomic<uint64_t> serial{0};
        st.serial = ++serial;
    }
    auto& st = *sp;
    // process_tiles_2d starts from zeros; the canvas may hold anything (the previous image, NaN): cleared through the buffer interface, never by arithmetic
    ggml_backend_tensor_memset(st.canvas, 0, 0, ggml_nbytes(st.canvas));

    Runner& r = dir == 1 ? ctx->vae_enc_runner : ctx->vae_runner;
    const size_t in_plane = (size_t)iw * ih, tile_plane = (size_t)itw * ith;
    std::vector<std::vector<float>> crops;  // kept until the read-back: uploads and graphs are enqueued, not waited for
    crops.reserve((size_t)(T + k - 1) / k);
    for (int t0 = 0; t0 < T; t0 += k) {
        const int kb       = std::min(k, T - t0);
        ggml_tensor* store = st.store[kb == k ? 0 : 1];
        // crop: [itw, ith, ic, n * kb], image-major (index n_i * kb + t): the ramp vectors [., ., 1, kb] then broadcast over the images like any ggml operand
        crops.emplace_back(tile_plane * ic * n * kb);
        float* cb = crops.back().data();
        for (int t = 0; t < kb; ++t) {
            const int x0 = pl.ax.pos[(t0 + t) % ntx].first * (decode ? 1 : scale), y0 = pl.ay.pos[(t0 + t) / ntx].first * (decode ? 1 : scale);
            for (int b = 0; b < n; ++b)
                for (int c = 0; c < ic; ++c) {
                    const float* src = in + ((size_t)b * ic + c) * in_plane + (size_t)y0 * iw + x0;
                    float* dst       = cb + (((size_t)b * kb + t) * ic + c) * tile_plane;
                    for (int y = 0; y < ith; ++y) memcpy(dst + (size_t)y * itw, src + (size_t)y * iw, (size_t)itw * sizeof(float));
                }
        }
        auto build = [&](GraphCtx& g, std::vector<HostInput>& inp) {
            g.flash_attn    = ctx->params.diffusion_flash_attn;
            g.conv_direct   = ctx->params.diffusion_conv_direct;
            ggml_tensor* tz = ggml_new_tensor_4d(g.ctx, GGML_TYPE_F32, itw, ith, ic, (int64_t)n * kb);
            ggml_set_input(tz);
            inp.push_back({tz, cb, ggml_nbytes(tz)});
            ggml_tensor* y = decode ? ctx->vae.forward(g, tz) : dir == 1 ? ctx->vae_enc.forward(g, tz) : tz;
            return ggml_cpy(g.ctx, y, store);  // tile positions stay out of this graph: every full batch replays one plan
        };
        char sig[128];
        snprintf(sig, sizeof(sig), "vae-tile%d %d %d %d %d*%d s%g #%llu", dir, itw, ith, ic, n, kb, (double)ctx->vae_conv2d_scale, (unsigned long long)st.serial);
        if (!r.compute(build, nullptr, 0, sig, {cb})) return false;

        // merge graph of this batch: MUL(tiles, wy) -> MUL(., wx) -> per tile, in processing order, ADD in place into the canvas behind the tile's skip
        ggml_init_params ip{0, nullptr, true};
        ggml_context* mc = ggml_init(ip);
        ggml_cgraph* gf  = ggml_new_graph_custom(mc, 64 + 4 * (size_t)kb, false);
        // (with both overlaps 0 every ramp value is s(1) = 1: the products are the tile's own bits, and the copies below store them like the reference does)
        ggml_tensor* wy = ggml_view_4d(mc, st.wy, 1, oth, 1, kb, st.wy->nb[1], st.wy->nb[2], st.wy->nb[3], (size_t)t0 * st.wy->nb[3]);
        ggml_tensor* wx = ggml_view_4d(mc, st.wx, otw, 1, 1, kb, st.wx->nb[1], st.wx->nb[2], st.wx->nb[3], (size_t)t0 * st.wx->nb[3]);
        ggml_tensor* m  = ggml_mul(mc, ggml_mul(mc, store, wy), wx);
        for (int t = 0; t < kb; ++t) {
            const auto& px = pl.ax.pos[(t0 + t) % ntx];
            const auto& py = pl.ay.pos[(t0 + t) / ntx];
            const int dx = px.second * om, dy = py.second * om, x = px.first * om, y = py.first * om;
            ggml_tensor* tv = ggml_view_4d(mc, m, otw - dx, oth - dy, oc, n, m->nb[1], m->nb[2], m->nb[3] * kb, (size_t)t * m->nb[3] + (size_t)dy * m->nb[1] + (size_t)dx * m->nb[0]);
            ggml_tensor* cv = ggml_view_4d(mc, st.canvas, otw - dx, oth - dy, oc, n, st.canvas->nb[1], st.canvas->nb[2], st.canvas->nb[3],
                                           (size_t)(y + dy) * st.canvas->nb[1] + (size_t)(x + dx) * st.canvas->nb[0]);
            ggml_build_forward_expand(gf, blend ? ggml_add_inplace(mc, cv, tv) : ggml_cpy(mc, tv, cv));
        }
        bool ok = ggml_gallocr_alloc_graph(st.merge_galloc, gf);
        if (!ok) set_error("VAE tiling: merge buffer allocation failed");
        if (ok && g_graph_capture) g_last_graph = describe_graph(gf);
        // (an installed eval callback sees the merge graphs like every other graph of the context: slices that cut the MUL / MUL / ADD chain run as plain nodes)
        if (ok && (g_eval_cb ? (enum ggml_status)sdm_backend_graph_compute_with_eval_callback(ctx->backend, gf, g_eval_cb, g_eval_cb_data)
                             : ggml_backend_graph_compute_async(ctx->backend, gf)) != GGML_STATUS_SUCCESS) {
            set_error("VAE tiling: merge graph compute failed");
            ok = false;
        }
        ggml_free(mc);
        if (!ok) return false;
    }
    ggml_backend_tensor_get(st.canvas, out, 0, ggml_nbytes(st.canvas));  // synchronises the stream
    if (r.galloc) ctx->stats.compute_buffer_bytes = ggml_gallocr_get_buffer_size(r.galloc, 0);
    return true;
}

void sdm_tiling_params_init(sdm_tiling_params_t* p) { *p = sdm_tiling_params_t{false, 0, 0, 0.5f, 0.f, 0.f, 0}; }
bool sd_set_vae_tiling(sdm_ctx_t* ctx, const sdm_tiling_params_t* params) {
    if (params && params->enabled && (params->tile_batch < 0 || !std::isfinite(params->target_overlap) || !std::isfinite(params->rel_size_x) || !std::isfinite(params->rel_size_y))) {
        set_error("sd_set_vae_tiling: tile_batch must be >= 0 and the overlap / relative sizes finite");
        return false;
    }
    if (params)
        ctx->tiling = *params;
    else
        sdm_tiling_params_init(&ctx->tiling);
    if (!ctx->tiling.enabled)
        for (auto& st : ctx->tstate) st.reset();
    return true;
}
bool sd_tiling_blend(sdm_ctx_t* ctx, const float* in, int w, int h, int c, int n, float* out) {
    if (!ctx->tiling.enabled || w < 1 || h < 1 || c < 1 || n < 1) {
        set_error("sd_tiling_blend: tiling is off (sd_set_vae_tiling) or the input is empty");
        return false;
    }
    return vae_tiled(ctx, 2, in, w, h, c, n, out);
}
int sd_tiling_plan(int small_w, int small_h, const sdm_tiling_params_t* params, float encode_factor, int* tile_size, int* overlap, int* tiles, int tile_capacity) {
    TilePlan pl;
    if (!params || !tiling_plan(small_w, small_h, *params, encode_factor, pl)) return -1;
    if (tile_size) tile_size[0] = pl.ax.tile, tile_size[1] = pl.ay.tile;
    if (overlap) overlap[0] = pl.ax.overlap, overlap[1] = pl.ay.overlap;
    const int T = pl.count(), ntx = (int)pl.ax.pos.size();
    for (int t = 0; tiles && t < T && t < tile_capacity; ++t) {
        tiles[4 * t + 0] = pl.ax.pos[t % ntx].first;
        tiles[4 * t + 1] = pl.ay.pos[t / ntx].first;
        tiles[4 * t + 2] = pl.ax.pos[t % ntx].second;
        tiles[4 * t + 3] = pl.ay.pos[t / ntx].second;
    }
    return T;
}

// ---- VAE decode ---------------------------------------------------------------------------------
bool sd_vae_decode_raw(sdm_ctx_t* ctx, const float* latents, int w, int h, int c, int n, float* out_rgb) {
    Runner& r       = ctx->vae_runner;
    const float sf  = ctx->vae.cfg.scale_factor, sh = ctx->vae.cfg.shift_factor;
    const size_t ne = (size_t)w * h * c * n;
    std::vector<float> z(ne);
    for (size_t i = 0; i < ne; ++i) z[i] = latents[i] / sf + sh;  // diffusion_to_vae_latents, auto_encoder_kl.hpp:818-826
    if (ctx->tiling.enabled) return vae_tiled(ctx, 0, z.data(), w, h, c, n, out_rgb);  // VAE::decode, vae.hpp:182-205
    auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
        g.flash_attn    = ctx->params.diffusion_flash_attn;
        g.conv_direct   = ctx->params.diffusion_conv_direct;
        ggml_tensor* tz = ggml_new_tensor_4d(g.ctx, GGML_TYPE_F32, w, h, c, n);
        ggml_set_input(tz);
        in.push_back({tz, z.data(), ggml_nbytes(tz)});
        return ctx->vae.forward(g, tz);
    };
    const size_t on = (size_t)w * 8 * h * 8 * 3 * n;
    char sig[64];
    snprintf(sig, sizeof(sig), "vae %d %d %d %d s%g", w, h, c, n, (double)ctx->vae_conv2d_scale);
    return r.compute(build, out_rgb, on * sizeof(float), sig, {z.data()});
}
bool sd_vae_decode(sdm_ctx_t* ctx, const float* latents, int w, int h, int c, int n, float* out_rgb) {
    const size_t on = (size_t)w * 8 * h * 8 * 3 * n;
    const double t0 = now_ms();
    if (!sd_vae_decode_raw(ctx, latents, w, h, c, n, out_rgb)) return false;
    parallel_chunks(on, [&](size_t b, size_t e) {  // scale_tensor_to_0_1, vae.hpp:24-30
        for (size_t i = b; i < e; ++i) {
            const float v = (out_rgb[i] + 1.0f) * 0.5f;
            out_rgb[i]    = std::max(0.0f, std::min(1.0f, v));
        }
    });
    ctx->stats.last_decode_ms = now_ms() - t0;
    return true;
}

// ---- VAE encode (the data format in front of the path: pixels -> the init latent of img2img) -------------
static bool ensure_vae_encoder(sdm_ctx_t* ctx) {
    if (ctx->vae_enc_ready) return true;
    Runner& r        = ctx->vae_enc_runner;
    r.backend        = ctx->backend;
    r.ps.linear_type = GGML_TYPE_F16;
    r.graph_size     = 20480;
    ctx->vae_enc.init(r.ps, "first_stage_model.", ctx->vae.cfg);
    ctx->vae_enc.set_conv2d_scale(ctx->vae_conv2d_scale);  // AutoEncoderKL::set_conv2d_scale reaches every Conv2d of the autoencoder, encoder included
    if (!r.alloc_weights(ctx->params.weight_seed)) {
        set_error("VAE encoder weight buffer allocation failed");
        return false;
    }
    for (auto& sp : r.ps.specs) ctx->all_tensors.push_back({sp.name, sp.tensor});
    ctx->stats.weight_bytes += ggml_backend_buffer_get_size(r.weights);
    ctx->vae_enc_ready = true;
    return true;
}
// encode_first_stage (stable-diffusion.cpp:3042-3060) = VAE::encode (vae.hpp:112-168: x * 2 - 1, the encoder graph -> moments), gaussian_latent_sample
// (auto_encoder_kl.hpp:750-759: mean + exp(0.5 * clamp(logvar, -30, 20)) * randn from the context RNG — seeded with the request's seed, offset 0, stable-diffusion.cpp:5630),
// vae_to_diffusion_latents ((z - shift) * scale, :830-838).  rgb: planar f32 [w, h, 3, n] in [0, 1]; w, h multiples of 8; out: [w/8, h/8, zc, n].
// moments_out (optional, 2 * zc channels): what left the graph.
bool sd_vae_encode(sdm_ctx_t* ctx, const float* rgb, int w, int h, int n, uint64_t seed, float* out_latents, float* moments_out) {
    if (w < 8 || h < 8 || w % 8 || h % 8 || n < 1) {
        set_error("sd_vae_encode: width and height must be positive multiples of 8");
        return false;
    }
    if (!ensure_vae_encoder(ctx)) return false;
    Runner& r       = ctx->vae_enc_runner;
    const size_t ni = (size_t)w * h * 3 * n;
    std::vector<float> x(ni);
    for (size_t i = 0; i < ni; ++i) x[i] = rgb[i] * 2.0f - 1.0f;  // scale_tensor_to_minus1_1, vae.hpp:17-22
    const int zc = (int)ctx->vae.cfg.z_channels, lw = w / 8, lh = h / 8;
    auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
        g.flash_attn    = ctx->params.diffusion_flash_attn;
        g.conv_direct   = ctx->params.diffusion_conv_direct;
        ggml_tensor* tx = ggml_new_tensor_4d(g.ctx, GGML_TYPE_F32, w, h, 3, n);
        ggml_set_input(tx);
        in.push_back({tx, x.data(), ggml_nbytes(tx)});
        return ctx->vae_enc.forward(g, tx);
    };
    const size_t plane = (size_t)lw * lh, per = plane * zc;
    std::vector<float> moments(2 * per * n);
    char sig[64];
    snprintf(sig, sizeof(sig), "vae-enc %d %d %d s%g", w, h, n, (double)ctx->vae_conv2d_scale);
    if (ctx->tiling.enabled) {  // VAE::encode, vae.hpp:130-154: the split follows x * 2 - 1; the sample and the latent scaling below see the merged moments
        if (!vae_tiled(ctx, 1, x.data(), w, h, 3, n, moments.data())) return false;
    } else if (!r.compute(build, moments.data(), moments.size() * sizeof(float), sig, {x.data()}))
        return false;
    if (moments_out) memcpy(moments_out, moments.data(), moments.size() * sizeof(float));
    if (ctx->variant == SDM_UNET_PIX2PIX && (ctx->params.model == SD_MODEL_SD15 || ctx->params.model == SD_MODEL_SD15_TINY)) {
        // VERSION_SD1_PIX2PIX: the latent is the mean of the moments (vae_output_to_latents, auto_encoder_kl.hpp:764-765), not sampled, and it is NOT scaled to the
        // diffusion range (encode_first_stage, stable-diffusion.cpp:3056-3058).  SDXL pix2pix takes the ordinary path below
        for (int b = 0; b < n; ++b) memcpy(out_latents + (size_t)b * per, &moments[(size_t)b * 2 * per], per * sizeof(float));
        return true;
    }
    PhiloxRNG rng(seed);
    const std::vector<float> noise = rng.randn((uint32_t)(per * n));  // randn_like(mean): one draw over the whole [lw, lh, zc, n] tensor
    const float sf = ctx->vae.cfg.scale_factor, sh = ctx->vae.cfg.shift_factor;
    for (int b = 0; b < n; ++b)
        for (size_t i = 0; i < per; ++i) {
            const float mean = moments[(size_t)b * 2 * per + i], logvar = moments[(size_t)b * 2 * per + per + i];
            const float stddev = std::exp(0.5f * std::max(-30.0f, std::min(20.0f, logvar)));
            const float z      = mean + stddev * noise[(size_t)b * per + i];
            out_latents[(size_t)b * per + i] = (z - sh) * sf;
        }
    return true;
}

// ---- TAESD decode ------------------------------------------------------
// TinyImageAutoEncoder (src/model/vae/tae.hpp:732-792; made at stable-diffusion.cpp:1407-1424 with the weights of `--taesd`, file prefix "tae."): parameters
// "tae.decoder.layers.<i>. ...", z_channels 16 for the DiT families.  Weights: synthetic like every other module until sd_load_weights_prefixed(ctx, file, "tae.") fills them.
static bool ensure_tae(sdm_ctx_t* ctx) {
    if (ctx->tae_ready) return true;
    Runner& r       = ctx->tae_runner;
    r.backend       = ctx->backend;
    r.ps.linear_type = GGML_TYPE_F16;
    r.graph_size    = 2048;
    ctx->tae.init(r.ps, "tae.decoder.layers.", ctx->is_dit ? 16 : 4);
    if (!r.alloc_weights(ctx->params.weight_seed)) {
        set_error("TAESD weight buffer allocation failed");
        return false;
    }
    for (auto& sp : r.ps.specs) ctx->all_tensors.push_back({sp.name, sp.tensor});
    ctx->stats.weight_bytes += ggml_backend_buffer_get_size(r.weights);
    ctx->tae_ready = true;
    return true;
}
// decode_first_stage with the tiny autoencoder: the diffusion latents enter as they are (diffusion_to_vae_latents is the identity, tae.hpp:763-765), the graph's output IS the
// image (scale_input = false, tae.hpp:745: no (x + 1) / 2, no clamp — the u8 conversion clamps); latents [w,h,zc,n] -> rgb f32 [8w,8h,3,n]
bool sd_tae_decode(sdm_ctx_t* ctx, const float* latents, int w, int h, int c, int n, float* out_rgb) {
    if (!ensure_tae(ctx)) return false;
    if (c != (int)ctx->tae.z_channels) {
        set_error("sd_tae_decode: the latents have " + std::to_string(c) + " channels, this model's TAESD takes " + std::to_string(ctx->tae.z_channels));
        return false;
    }
    Runner& r  = ctx->tae_runner;
    auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
        g.conv_direct   = ctx->params.diffusion_conv_direct;
        ggml_tensor* tz = ggml_new_tensor_4d(g.ctx, GGML_TYPE_F32, w, h, c, n);
        ggml_set_input(tz);
        in.push_back({tz, latents, ggml_nbytes(tz)});
        return ctx->tae.forward(g, tz);
    };
    const size_t on = (size_t)w * 8 * h * 8 * 3 * n;
    const double t0 = now_ms();
    char sig[64];
    snprintf(sig, sizeof(sig), "tae %d %d %d %d", w, h, c, n);
    if (!r.compute(build, out_rgb, on * sizeof(float), sig, {latents})) return false;
    ctx->stats.last_decode_ms = now_ms() - t0;
    return true;
}
// the reference decodes with TAESD instead of the KL-VAE when a taesd file is given and it is not for previews only (stable-diffusion.cpp:1496-1516): sdm_generate_image's switch
// sd_ctx_params_t::prediction (stable-diffusion.h prediction_t; resolved at stable-diffusion.cpp:1760-1790): v-prediction UNets (SD2.x 768-v, v-pred SDXL fine-tunes) use
// CompVisVDenoiser's scalings; the flow families have one parameterisation each
bool sd_set_prediction(sdm_ctx_t* ctx, int prediction) {
    if (prediction != SDM_EPS_PRED && prediction != SDM_V_PRED) {
        set_error("sd_set_prediction: only SDM_EPS_PRED and SDM_V_PRED are implemented");
        return false;
    }
    if (ctx->is_dit && prediction != SDM_EPS_PRED) {
        set_error("sd_set_prediction: the flow families (SD3.x, FLUX) have a fixed parameterisation");
        return false;
    }
    ctx->prediction = prediction;
    return true;
}
bool sd_use_tae(sdm_ctx_t* ctx, bool on) {
    if (on && !ensure_tae(ctx)) return false;
    ctx->tae_for_images = on;
    return true;
}

// ---- latent previews (csrc/host/preview.hpp) ----------------------------------------------------------------
// The two byte stages (include/ggml-mi355x.h) as the samplers and sdm_latent_preview / sdm_planar_to_u8 reach them: plug-in exports found through the registry's
// get_proc_address, enqueued on the backend's stream.  A backend without them (the CPU oracle of the tests) takes the host restatement; the product backend
// without them is an error at sampling time, never a quiet fall-back (the step caches' rule).
struct PreviewDevice {
    typedef bool (*proj_fn)(ggml_backend_t, const float*, int64_t, int, int64_t, float, const float*, const float*, uint8_t*);
    typedef bool (*u8_fn)(ggml_backend_t, const float*, int64_t, int64_t, float, float, uint8_t*);
    ggml_backend_t backend = nullptr;
    proj_fn proj_k         = nullptr;
    u8_fn u8_k             = nullptr;
    bool exports_missing   = false;
    explicit PreviewDevice(ggml_backend_t be) : backend(be) {
        ggml_backend_dev_t dev = ggml_backend_get_device(be);
        ggml_backend_reg_t reg = dev ? ggml_backend_dev_backend_reg(dev) : nullptr;
        if (reg) {
            proj_k = (proj_fn)ggml_backend_reg_get_proc_address(reg, "ggml_backend_mi355x_latent_preview");
            u8_k   = (u8_fn)ggml_backend_reg_get_proc_address(reg, "ggml_backend_mi355x_planar_to_u8");
        }
        if (!proj_k || !u8_k) proj_k = nullptr, u8_k = nullptr;
        exports_missing = !proj_k && reg && strcmp(ggml_backend_reg_name(reg), "MI355X") == 0;
    }
    bool on_device() const { return proj_k != nullptr; }
    // t: [plane, c, n] f32 on the backend -> out (host bytes, complete on return: the one synchronisation of a preview)
    bool latent(ggml_tensor* t, int64_t plane, int c, int64_t n, float in_scale, const float* proj, const float* bias, uint8_t* out, std::vector<float>& tmp) {
        if (proj_k) {
            const bool ok = proj_k(backend, (const float*)t->data, plane, c, n, in_scale, proj, bias, out);
            ggml_backend_synchronize(backend);
            return ok;
        }
        tmp.resize((size_t)(plane * c * n));
        ggml_backend_tensor_get(t, tmp.data(), 0, tmp.size() * sizeof(float));
        return latent_preview_host(tmp.data(), plane, c, n, in_scale, proj, bias, out);
    }
};
// the projection of a c-channel latent on this context: the installed table when it fits, else the family's, else (3 channels) none; false: no table known
static bool preview_table(const sdm_ctx_t* ctx, int c, const float** proj, const float** bias) {
    const PreviewState& pv = ctx->preview;
    if (pv.custom_c == c && !pv.custom_proj.empty()) {
        *proj = pv.custom_proj.data(), *bias = pv.custom_bias;
        return true;
    }
    const PreviewTable ft = preview_family_table(ctx->params.model);
    if (ft.channels == c) {
        *proj = &ft.proj[0][0], *bias = ft.bias;
        return true;
    }
    *proj = nullptr, *bias = nullptr;
    return c == 3;
}
// the PROJ pass over host memory through the path the sampler uses: upload + kernel on a backend with the exports, the restatement otherwise
static bool preview_proj_host_latent(sdm_ctx_t* ctx, PreviewDevice& dev, const float* x, int w, int h, int c, int n, float in_scale, const float* proj, const float* bias,
                                     uint8_t* out) {
    const int64_t plane = (int64_t)w * h;
    if (!dev.on_device()) return latent_preview_host(x, plane, c, n, in_scale, proj, bias, out);
    auto& up = ctx->preview_upload;
    if (!up || up->latent->ne[0] != w || up->latent->ne[1] != h || up->latent->ne[2] != c || up->latent->ne[3] != n) {
        up.reset(new sdm_ctx_t::PreviewUpload());
        ggml_init_params ip{0, nullptr, true};
        up->cctx   = ggml_init(ip);
        up->latent = ggml_new_tensor_4d(up->cctx, GGML_TYPE_F32, w, h, c, n);
        ggml_set_name(up->latent, "preview.latent");
        up->buf = ggml_backend_alloc_ctx_tensors(up->cctx, ctx->backend);
        if (!up->buf) {
            up.reset();
            set_error("preview: upload buffer allocation failed");
            return false;
        }
    }
    ggml_backend_tensor_set_async(ctx->backend, up->latent, x, 0, (size_t)plane * c * n * sizeof(float));
    std::vector<float> unused;
    return dev.latent(up->latent, plane, c, n, in_scale, proj, bias, out, unused);
}
// One preview of the current device group: host (host loop) or dev (device-resident sampler) holds the latent [W, H, C, nb]; in_scale != 1 only for the device sampler's
// noisy preview (x, c_in).  Runs the mode's byte stage, hands the callback nb frames.  false (error set): the pass could not be run.
static bool emit_preview(sdm_ctx_t* ctx, int step, bool is_noisy, int b0, int W, int H, int C, int nb, const float* host, ggml_tensor* dev, float in_scale) {
    PreviewState& pv = ctx->preview;
    PreviewDevice pd(ctx->backend);
    if (pd.exports_missing) {
        set_error("preview: the MI355X backend does not export its preview passes (ggml_backend_mi355x_latent_preview / _planar_to_u8)");
        return false;
    }
    const size_t n = (size_t)W * H * C * nb;
    int FW = W, FH = H;
    bool ok = true;
    if (pv.mode == SDM_PREVIEW_PROJ) {
        const float *proj, *bias;
        if (!preview_table(ctx, C, &proj, &bias)) {
            set_error("preview: no latent to RGB projection known for " + std::to_string(C) + " channels (sdm_set_preview_projection)");
            return false;
        }
        pv.bytes.resize((size_t)W * H * 3 * nb);
        ok = dev ? pd.latent(dev, (int64_t)W * H, C, nb, in_scale, proj, bias, pv.bytes.data(), pv.staging)
                 : preview_proj_host_latent(ctx, pd, host, W, H, C, nb, in_scale, proj, bias, pv.bytes.data());
        if (!ok) set_error("preview: the projection pass could not be run");
    } else {
        // the decode modes: the (small) latent comes to the host, the decoders' entry points run their graphs, the image stays on the device until the byte stage has
        // converted it — except through the tiling driver, whose canvas is read back as f32 and converted with the same arithmetic on the host
        std::vector<float> lat;
        const float* z = host;
        if (dev) {
            lat.resize(n);
            ggml_backend_tensor_get(dev, lat.data(), 0, n * sizeof(float));
            if (in_scale != 1.0f)
                for (size_t k = 0; k < n; ++k) lat[k] = lat[k] * in_scale;
            z = lat.data();
        }
        FW = W * 8, FH = H * 8;
        const int64_t plane = (int64_t)FW * FH;
        const bool tae      = pv.mode == SDM_PREVIEW_TAE;
        const float mul = tae ? 1.0f : 0.5f, add = tae ? 0.0f : 0.5f;  // VAE::decode's (x + 1) / 2 (vae.hpp:216-218) folded into the byte stage; TAESD's output is the image
        pv.bytes.resize((size_t)plane * 3 * nb);
        if (pd.on_device() && (tae || !ctx->tiling.enabled)) {
            Runner& r = tae ? ctx->tae_runner : ctx->vae_runner;
            ok        = tae ? sd_tae_decode(ctx, z, W, H, C, nb, nullptr) : sd_vae_decode_raw(ctx, z, W, H, C, nb, nullptr);  // (no output buffer: enqueued, nothing read back)
            if (ok && r.last_res_bytes != (size_t)plane * 3 * nb * sizeof(float)) {
                set_error("preview: decode output size mismatch");
                ok = false;
            }
            if (ok && !pd.u8_k(ctx->backend, (const float*)r.last_res_data, plane, nb, mul, add, pv.bytes.data())) {
                set_error("preview: the byte pass could not be enqueued");
                ok = false;
            }
            ggml_backend_synchronize(ctx->backend);
        } else {
            pv.staging.resize((size_t)plane * 3 * nb);
            ok = tae ? sd_tae_decode(ctx, z, W, H, C, nb, pv.staging.data()) : sd_vae_decode_raw(ctx, z, W, H, C, nb, pv.staging.data());
            ok = ok && planar_to_u8_host(pv.staging.data(), plane, nb, mul, add, pv.bytes.data());
        }
    }
    if (!ok) return false;
    std::vector<sdm_image_t> frames((size_t)nb);
    for (int b = 0; b < nb; ++b) frames[(size_t)b] = sdm_image_t{(uint32_t)FW, (uint32_t)FH, 3, pv.bytes.data() + (size_t)b * FW * FH * 3};
    struct Current {  // what sdm_preview_first_image / sdm_preview_latent answer with while the callback runs
        sdm_ctx_t* ctx;
        ~Current() { ctx->preview_current = sdm_ctx_t::PreviewCurrent(); }
    } current{ctx};
    ctx->preview_current = sdm_ctx_t::PreviewCurrent{true, b0, host, dev, (int64_t)n, in_scale};
    pv.cb(step, nb, frames.data(), is_noisy, pv.user);
    return true;
}

// ---- sample(): the denoise loop -------------------------------------------------------------------
// resolve_sample_method / sd_get_default_sample_method (stable-diffusion.cpp:3965-3975, 4006-4013): DiT families default to plain Euler
static int resolve_sample_method(const sdm_ctx_t* ctx, int m) {
    if (m == SDM_SAMPLE_METHOD_COUNT) return ctx->is_dit ? SDM_EULER_SAMPLE_METHOD : SDM_EULER_A_SAMPLE_METHOD;
    return m;
}
// resolve_scheduler / sd_get_default_scheduler (stable-diffusion.cpp:3977-3998, 4015-4022)
static int resolve_scheduler(const sdm_ctx_t* ctx, int scheduler, int method) {
    if (scheduler != SDM_SCHEDULER_COUNT) return scheduler;
    if (method == SDM_LCM_SAMPLE_METHOD || method == SDM_TCD_SAMPLE_METHOD) return SDM_LCM_SCHEDULER;
    if (method == SDM_DDIM_TRAILING_SAMPLE_METHOD) return SDM_SIMPLE_SCHEDULER;
    return ctx->is_flux ? SDM_FLUX_SCHEDULER : SDM_DISCRETE_SCHEDULER;
}
// method / scheduler / eta of one call, resolved as generate_image does (resolve_sample_method, resolve_scheduler, resolve_eta: stable-diffusion.cpp:4006-4049).  DDIM trailing IS
// Euler-A on the reference (sample_k_diffusion, denoiser.hpp:2843-2845) with its own eta / scheduler defaults: `method` comes back as Euler-A for it.
static bool resolve_sampling(const sdm_ctx_t* ctx, const sdm_sample_params_t& sp, int& method, int& scheduler, float& eta) {
    method    = resolve_sample_method(ctx, sp.sample_method);
    scheduler = resolve_scheduler(ctx, sp.scheduler, method);
    if (!sample_method_supported(method)) {
        set_error("sample method " + std::to_string(method) + " is not implemented (sdm_sample_method_t: 0 ... 20)");
        return false;
    }
    if (!scheduler_supported(scheduler)) {
        set_error("scheduler " + std::to_string(scheduler) + " is not implemented (sdm_scheduler_t)");
        return false;
    }
    eta = sp.eta == INFINITY ? default_eta(method) : sp.eta;
    if (method == SDM_DDIM_TRAILING_SAMPLE_METHOD) method = SDM_EULER_A_SAMPLE_METHOD;
    return true;
}
// scalings and timestep of one model call: Denoiser::get_scalings + sigma_to_t, and — sd_sample_params_t::shifted_timestep > 0 (timestep-shifted distilled UNets) —
// prepare_sample_timesteps / adjust_sample_step_scalings (stable-diffusion.cpp:2411-2457): the model sees round(t * shift / 1000) and the output scalings of THAT timestep's sigma
static void step_scalings(const sdm_ctx_t* ctx, const sdm_sample_params_t& sp, float sigma, float& c_skip, float& c_out, float& c_in, float& t) {
    ctx->scalings(sigma, c_skip, c_out, c_in);
    t = ctx->sigma_to_t(sigma);
    if (sp.shifted_timestep > 0 && !ctx->is_dit) {
        const float shifted_t_float = t * (float(sp.shifted_timestep) / float(TIMESTEPS));
        int64_t shifted_t           = static_cast<int64_t>(roundf(shifted_t_float));
        shifted_t                   = std::max((int64_t)0, std::min((int64_t)(TIMESTEPS - 1), shifted_t));
        t                           = (float)shifted_t;
        const int64_t idx           = static_cast<int64_t>(roundf(t));
        const float shifted_sigma   = ctx->denoiser.t_to_sigma((float)idx);
        float s_skip, s_out, s_in;
        ctx->scalings(shifted_sigma, s_skip, s_out, s_in);
        c_skip = s_skip * c_in / s_in;
        c_out  = s_out;
    }
}
// Which model evaluations a denoise call makes — resolve_guidance, stable-diffusion.cpp:4237-4255: img_cfg unset = 1; a model without image conditioning ignores it;
// the uncond branch runs iff img_cfg != txt_cfg (with img_cfg 1: txt_cfg != 1), the img_uncond branch iff img_cfg != 1.  Both need the uncond conditioning (its text
// is the third condition's text too)
struct GuidancePlan {
    float img_cfg       = 1.0f;
    bool use_uncond     = false;
    bool use_img_uncond = false;
    int branches() const { return 1 + (int)use_uncond + (int)use_img_uncond; }
};
static GuidancePlan resolve_guidance_plan(const sdm_ctx_t* ctx, const sdm_img_gen_params_t* p) {
    GuidancePlan gp;
    gp.img_cfg = (std::isfinite(ctx->img_cfg) && ctx->variant != SDM_UNET_PLAIN) ? ctx->img_cfg : 1.0f;
    const bool has_uncond = p->uncond.c_crossattn != nullptr;
    gp.use_uncond         = gp.img_cfg != p->sample_params.txt_cfg && has_uncond;
    gp.use_img_uncond     = gp.img_cfg != 1.0f && has_uncond;
    return gp;
}
// the concat condition of the device group (b0, nb): shared by the batch (n = 1, the reference's case) or the group's slice of a per-image one
static void group_concat(const sdm_ctx_t* ctx, int b0, int nb, const float*& concat, const float*& img_concat, int& cc, int& concat_n) {
    const sdm_ctx_t::ConcatCondition& s = ctx->concat_cond;
    concat = img_concat = nullptr;
    cc = concat_n = 0;
    if (!s.set() || ctx->variant == SDM_UNET_PLAIN) return;
    const size_t one = (size_t)s.w * s.h * s.cc;
    const size_t off = s.n == 1 ? 0 : one * (size_t)b0;
    concat     = s.concat.data() + off;
    img_concat = s.img_uncond.data() + off;
    cc         = s.cc;
    concat_n   = s.n == 1 ? 1 : nb;
}
// One denoiser call of the host loop — the reference's `denoise` lambda (stable-diffusion.cpp:2620-2926) on nb images: scalings and timestep of sigma, x * c_in, the model
// forward(s) (the cond / uncond pair in ONE graph when the conditionings allow it), classifier-free guidance, pred * c_out + x * c_skip.
struct HostDenoise {
    sdm_ctx_t* ctx;
    const sdm_img_gen_params_t* p;
    int W, H, C, nb;
    size_t per;
    bool use_cfg;
    std::vector<float> noised, cond_out, uncond_out, ts, skip_out;
    int n_sigmas = 0;  // sigmas.size() of the trajectory (GuidanceInput::schedule_size)
    std::vector<std::vector<float>> apg_momentum;  // adaptive projected guidance: one momentum buffer per image
    std::vector<float> x2, o2, t2, c2, y2;  // staging of the fused (cond, uncond) pair
    std::vector<float> ip2;                 // ... and its image tokens [ip_dim, n_ip, K] (sd_set_ip_adapter), assembled on first use
    // step cache (csrc/host/step_cache.hpp): every model forward is wrapped like the reference's run_condition (stable-diffusion.cpp:2779-2795), cond = 0 and
    // uncond = 1; the input is `noised` and the output the model output over the whole device group (nb = 1: the reference's tensors; nb > 1: the means run over
    // the group and there is one decision for all its images)
    StepCacheRuntime* sc = nullptr;
    HostStepCacheStore sc_store;
    std::vector<float> spectrum_ring;  // Spectrum's H_buf: K slots of the group's denoised tensor (SpectrumState keeps which slot is which)
    // c_concat and image guidance (sd_set_concat_condition / sd_set_img_cfg; inpaint and pix2pix UNets): cond and uncond both see `concat`, the third condition is
    // uncond's text with `img_concat` (stable-diffusion.cpp:5236-5237, 5265-5266, 5273).  Branches as resolve_guidance (:4249-4255) sets them; with no concat
    // condition and img_cfg 1 everything below is exactly the two-branch loop
    GuidancePlan gp;
    const float *concat = nullptr, *img_concat = nullptr;  // this group's [W, H, cc, concat_n]
    int cc = 0, concat_n = 0;
    std::vector<float> img_uncond_out, cc2;
    HostDenoise(sdm_ctx_t* ctx_, const sdm_img_gen_params_t* p_, int W_, int H_, int C_, int nb_, int b0_ = 0)
        : ctx(ctx_), p(p_), W(W_), H(H_), C(C_), nb(nb_), per((size_t)W_ * H_ * C_), use_cfg(false), noised(per * nb_), cond_out(per * nb_), uncond_out(per * nb_), ts(nb_) {
        gp      = resolve_guidance_plan(ctx, p);
        use_cfg = gp.use_uncond;
        group_concat(ctx, b0_, nb_, concat, img_concat, cc, concat_n);
        if (gp.use_img_uncond) img_uncond_out.resize(per * nb_);
    }
    // denoised_uncond (the CFG++ methods): GuiderOutput::pred_uncond = base_uncond * c_out + x * c_skip with the unconditional forward — or the conditional one when there is
    // no guidance pair (stable-diffusion.cpp:2877-2884)
    // step: the sampler's step index of this call (sample_k_diffusion hands the denoise callback i + 1, negated for the first stage of the two-stage methods): what
    // SkipLayerGuidance::is_enabled_for_step looks at (guidance.cpp:306-314)
    bool operator()(const float* x, float sigma, float* denoised, float* denoised_uncond = nullptr, int step = 0) {
        const sdm_sample_params_t& sp = p->sample_params;
        const size_t n = per * (size_t)nb;
        float c_skip, c_out, c_in, t;
        step_scalings(ctx, sp, sigma, c_skip, c_out, c_in, t);
        for (int b = 0; b < nb; ++b) ts[b] = t;
        for (size_t k = 0; k < n; ++k) noised[k] = x[k] * c_in;  // stable-diffusion.cpp:2662
        // Spectrum (stable-diffusion.cpp:2667-2679): a predicted call writes the forecast and returns — no forward, no guidance; only the inpainting blend follows
        const bool spectrum = sc && sc->spectrum_enabled;
        if (spectrum && sc->spectrum_begin_call(step, sigma)) {
            float weights[SpectrumState::MAX_K];
            int order[SpectrumState::MAX_K];
            const int k = sc->spectrum.predict(weights, order);
            spectrum_predict_host(spectrum_ring.data(), n, order, k, weights, sc->spectrum.config.w, n, denoised);
            blend_mask(denoised);
            return preview(step, false, denoised);  // stable-diffusion.cpp:2672-2674 (a forecast call never reaches the noisy preview)
        }
        if (!preview(step, true, noised.data())) return false;  // stable-diffusion.cpp:2681-2683
        const bool cached = sc && sc->armed();
        if (cached) sc->begin_call(step, sigma);  // SampleStepCacheDispatcher step_cache(cache_runtime, step, sigma), stable-diffusion.cpp:2688
        // image tokens (sd_set_ip_adapter): the cond branch sees the tokens, every other branch the uncond tokens (stable-diffusion.cpp:2829-2843); a forward of K
        // adjacent branches per image takes [tokens, uncond (, uncond)], tiled over the images like its context
        struct IpScope {
            sdm_ctx_t* c;
            IpScope(sdm_ctx_t* c_, const std::vector<float>* rows, int ip_n) : c(c_) {
                if (rows) c->ip_call = {rows->data(), ip_n};
            }
            ~IpScope() { c->ip_call = {}; }
        };
        const bool ip_on = ctx->ip_active();
        auto run = [&](const sd_condition_t& cd, float* dst, const float* cat = nullptr) {
            const int cond_id = &cd == &p->uncond ? 1 : 0;
            if (cached && sc_store.before_condition(*sc, cond_id, noised.data(), dst, n)) return true;
            IpScope ips(ctx, ip_on ? (cond_id == 0 ? &ctx->ip_tokens : &ctx->ip_uncond) : nullptr, 1);
            if (cat ? !sd_unet_forward_concat(ctx, noised.data(), W, H, C, nb, ts.data(), cd.c_crossattn, cd.ctx_dim, cd.n_tokens, 1, cd.c_vector, cd.vector_dim, 1, cat, cc, concat_n, dst)
                    : !sd_unet_forward(ctx, noised.data(), W, H, C, nb, ts.data(), cd.c_crossattn, cd.ctx_dim, cd.n_tokens, 1, cd.c_vector, cd.vector_dim, 1, dst))
                return false;
            if (cached) sc_store.after_condition(*sc, cond_id, noised.data(), dst, n);
            return true;
        };
        // the combine of the branches that ran (ClassifierFreeGuidance::forward, guidance.cpp:162-176; sd_cfg_combine3's arithmetic)
        auto guide3 = [&](float* dst) {
            if (gp.use_uncond)
                for (size_t k = 0; k < n; ++k) dst[k] = cfg_guided3(cond_out[k], uncond_out[k], img_uncond_out[k], sp.txt_cfg, gp.img_cfg);
            else
                for (size_t k = 0; k < n; ++k) dst[k] = cfg_guided(cond_out[k], img_uncond_out[k], sp.txt_cfg);
        };
        // the primary guidance of the (cond, uncond) pair: classifier-free (guidance.cpp:171) or, with any apg_* parameter set, adaptive projected guidance per image
        // (guidance.cpp:209-294; the momentum buffer lives as long as the trajectory, like the reference's guider object)
        auto guide = [&](float* dst) {
            const ApgParams apg{sp.apg_eta, sp.apg_momentum, sp.apg_norm_threshold, sp.apg_norm_threshold_smoothing};
            if (apg.enabled()) {
                if (apg_momentum.size() != (size_t)nb) apg_momentum.assign((size_t)nb, std::vector<float>());
                for (int b = 0; b < nb; ++b) apg_guided(&cond_out[(size_t)b * per], &uncond_out[(size_t)b * per], per, sp.txt_cfg, apg, apg_momentum[(size_t)b], dst + (size_t)b * per);
            } else {
                for (size_t k = 0; k < n; ++k) dst[k] = cfg_guided(cond_out[k], uncond_out[k], sp.txt_cfg);
            }
        };
        const int K = gp.branches();
        if (concat && K >= 2 && p->fuse_cfg_pair && p->cond.ctx_dim == p->uncond.ctx_dim && p->cond.n_tokens == p->uncond.n_tokens) {
            // one graph for the K = 2 or 3 evaluations of every image, interleaved (b cond, b uncond, b img_uncond): context / y have batch K and are tiled by the
            // graph's ggml_repeat; the concat has batch K (shared by the images: tiled the same way) or K * nb (per image)
            const size_t cn  = (size_t)p->cond.ctx_dim * p->cond.n_tokens;
            const bool has_y = p->cond.c_vector && p->uncond.c_vector;
            const size_t ccper = (size_t)W * H * cc;
            const int img_seat = gp.use_img_uncond ? K - 1 : -1;
            if (x2.empty()) {
                x2.resize((size_t)K * per * nb);
                o2.resize((size_t)K * per * nb);
                t2.resize((size_t)K * nb);
                c2.resize((size_t)K * cn);
                if (has_y) y2.resize((size_t)K * p->cond.vector_dim);
                for (int j = 0; j < K; ++j) {
                    const sd_condition_t& cd = j == 0 ? p->cond : p->uncond;
                    memcpy(&c2[(size_t)j * cn], cd.c_crossattn, cn * sizeof(float));
                    if (has_y) memcpy(&y2[(size_t)j * p->cond.vector_dim], cd.c_vector, p->cond.vector_dim * sizeof(float));
                }
                const int rows = concat_n == 1 ? 1 : nb;
                cc2.resize((size_t)K * rows * ccper);
                for (int b = 0; b < rows; ++b)
                    for (int j = 0; j < K; ++j)
                        memcpy(&cc2[((size_t)b * K + j) * ccper], (j == img_seat ? img_concat : concat) + (size_t)b * ccper, ccper * sizeof(float));
            }
            std::fill(t2.begin(), t2.end(), t);
            // (a cache is armed with the cond / uncond pair only: the third branch is refused together with it)
            if (cached && sc_store.before_condition(*sc, 0, noised.data(), cond_out.data(), n)) {
                if (!sc_store.before_condition(*sc, 1, noised.data(), uncond_out.data(), n)) {
                    set_error("step cache: no stored difference for the unconditional branch of a skipped step");
                    return false;
                }
            } else {
                for (int b = 0; b < nb; ++b)
                    for (int j = 0; j < K; ++j) memcpy(&x2[((size_t)K * b + j) * per], &noised[(size_t)b * per], per * sizeof(float));
                if (ip_on && ip2.empty()) ip2 = ctx->ip_rows(K);
                IpScope ips(ctx, ip_on ? &ip2 : nullptr, K);
                if (!sd_unet_forward_concat(ctx, x2.data(), W, H, C, K * nb, t2.data(), c2.data(), p->cond.ctx_dim, p->cond.n_tokens, K, has_y ? y2.data() : nullptr,
                                            p->cond.vector_dim, K, cc2.data(), cc, concat_n == 1 ? K : K * nb, o2.data()))
                    return false;
                for (int b = 0; b < nb; ++b) {
                    int j = 0;
                    memcpy(&cond_out[(size_t)b * per], &o2[((size_t)K * b + j++) * per], per * sizeof(float));
                    if (gp.use_uncond) memcpy(&uncond_out[(size_t)b * per], &o2[((size_t)K * b + j++) * per], per * sizeof(float));
                    if (gp.use_img_uncond) memcpy(&img_uncond_out[(size_t)b * per], &o2[((size_t)K * b + j++) * per], per * sizeof(float));
                }
                if (cached) {
                    sc_store.after_condition(*sc, 0, noised.data(), cond_out.data(), n);
                    sc_store.after_condition(*sc, 1, noised.data(), uncond_out.data(), n);
                }
            }
            if (gp.use_img_uncond)
                guide3(denoised);
            else
                guide(denoised);
        } else if (concat) {
            if (!run(p->cond, cond_out.data(), concat)) return false;
            if (gp.use_uncond && !run(p->uncond, uncond_out.data(), concat)) return false;
            if (gp.use_img_uncond && !run(p->uncond, img_uncond_out.data(), img_concat)) return false;
            if (gp.use_img_uncond)
                guide3(denoised);
            else if (gp.use_uncond)
                guide(denoised);
            else
                for (size_t k = 0; k < n; ++k) denoised[k] = cond_out[k];
        } else if (use_cfg && p->fuse_cfg_pair && p->cond.ctx_dim == p->uncond.ctx_dim && p->cond.n_tokens == p->uncond.n_tokens) {
            // one graph for the cond/uncond pair: images interleaved (b cond, b uncond, ...); context/y have batch 2 and are
            // tiled over the 2*nb images by the graph's ggml_repeat (dst[i] = src[i % 2])
            const size_t cn  = (size_t)p->cond.ctx_dim * p->cond.n_tokens;
            const bool has_y = p->cond.c_vector && p->uncond.c_vector;
            if (x2.empty()) {  // first call: the pair's conditioning is the same for every step, the staging buffers are reused
                x2.resize(2 * per * nb);
                o2.resize(2 * per * nb);
                t2.resize(2 * nb);
                c2.resize(2 * cn);
                memcpy(&c2[0], p->cond.c_crossattn, cn * sizeof(float));
                memcpy(&c2[cn], p->uncond.c_crossattn, cn * sizeof(float));
                if (has_y) {
                    y2.resize(2 * p->cond.vector_dim);
                    memcpy(&y2[0], p->cond.c_vector, p->cond.vector_dim * sizeof(float));
                    memcpy(&y2[p->cond.vector_dim], p->uncond.c_vector, p->cond.vector_dim * sizeof(float));
                }
            }
            std::fill(t2.begin(), t2.end(), t);
            // the anchor's before_condition runs in front of the ONE graph: on a skip both outputs come from their stored differences, otherwise the pair is
            // computed and after_condition sees cond, then uncond
            if (cached && sc_store.before_condition(*sc, 0, noised.data(), cond_out.data(), n)) {
                if (!sc_store.before_condition(*sc, 1, noised.data(), uncond_out.data(), n)) {
                    set_error("step cache: no stored difference for the unconditional branch of a skipped step");
                    return false;
                }
            } else {
                for (int b = 0; b < nb; ++b) {
                    memcpy(&x2[(2 * b) * per], &noised[b * per], per * sizeof(float));
                    memcpy(&x2[(2 * b + 1) * per], &noised[b * per], per * sizeof(float));
                }
                if (ip_on && ip2.empty()) ip2 = ctx->ip_rows(2);
                IpScope ips(ctx, ip_on ? &ip2 : nullptr, 2);
                if (!sd_unet_forward(ctx, x2.data(), W, H, C, 2 * nb, t2.data(), c2.data(), p->cond.ctx_dim, p->cond.n_tokens, 2,
                                     has_y ? y2.data() : nullptr, p->cond.vector_dim, 2, o2.data()))
                    return false;
                for (int b = 0; b < nb; ++b) {
                    memcpy(&cond_out[b * per], &o2[(2 * b) * per], per * sizeof(float));
                    memcpy(&uncond_out[b * per], &o2[(2 * b + 1) * per], per * sizeof(float));
                }
                if (cached) {
                    sc_store.after_condition(*sc, 0, noised.data(), cond_out.data(), n);  // (uncond's before_condition in between changes nothing: it is never the anchor)
                    sc_store.after_condition(*sc, 1, noised.data(), uncond_out.data(), n);
                }
            }
            guide(denoised);
        } else if (!run(p->cond, cond_out.data())) {
            return false;
        } else if (use_cfg) {
            if (!run(p->uncond, uncond_out.data())) return false;
            guide(denoised);
        } else {
            for (size_t k = 0; k < n; ++k) denoised[k] = cond_out[k];
        }
        // skip-layer guidance (SkipLayerGuidance, guidance.cpp:296-340; stable-diffusion.cpp:2593-2611, 2860-2871): inside the step window one more conditional forward
        // WITHOUT the listed joint blocks; guided += (cond - skip) * scale.  DiT families only (the reference warns and ignores it elsewhere)
        if (ctx->is_dit && !ctx->is_flux && sp.slg_scale != 0.0f && sp.slg_layers && sp.slg_layer_count > 0) {
            const size_t schedule_size = (size_t)n_sigmas;
            const int start_step = static_cast<int>(sp.slg_layer_start * static_cast<float>(schedule_size));
            const int stop_step  = static_cast<int>(sp.slg_layer_end * static_cast<float>(schedule_size));
            if (schedule_size != 0 && step > start_step && step < stop_step) {
                const std::vector<int> skip(sp.slg_layers, sp.slg_layers + sp.slg_layer_count);
                skip_out.resize(n);
                if (!unet_forward_skip(ctx, noised.data(), W, H, C, nb, ts.data(), p->cond.c_crossattn, p->cond.ctx_dim, p->cond.n_tokens, 1, p->cond.c_vector, p->cond.vector_dim, 1,
                                       skip_out.data(), &skip))
                    return false;
                for (size_t k = 0; k < n; ++k) {
                    volatile float d = cond_out[k] - skip_out[k];  // (three separately rounded operations, like cfg_guided)
                    volatile float sc = d * sp.slg_scale;
                    denoised[k] += sc;
                }
            }
        }
        for (size_t k = 0; k < n; ++k) denoised[k] = denoised[k] * c_out + x[k] * c_skip;  // stable-diffusion.cpp:2876
        if (denoised_uncond) {
            // base_uncond: img_uncond first, then uncond, then cond (stable-diffusion.cpp:2880-2882)
            const float* base = (concat && gp.use_img_uncond) ? img_uncond_out.data() : (use_cfg ? uncond_out.data() : cond_out.data());
            for (size_t k = 0; k < n; ++k) denoised_uncond[k] = base[k] * c_out + x[k] * c_skip;
        }
        if (spectrum) {  // SpectrumState::update in front of the mask blend (stable-diffusion.cpp:2885-2887)
            spectrum_ring.resize((size_t)sc->spectrum.K * n);
            memcpy(&spectrum_ring[(size_t)sc->spectrum.update() * n], denoised, n * sizeof(float));
        }
        blend_mask(denoised);
        return preview(step, false, denoised);  // stable-diffusion.cpp:2888-2892
    }
    // sd_set_preview_callback's hook: nothing happens (no tensor, no launch) unless a callback is installed and this call is due (csrc/host/preview.hpp)
    int b0 = 0;  // batch index of the group's first image
    bool preview(int step, bool is_noisy, const float* latent) { return !ctx->preview.wants(step, is_noisy) || emit_preview(ctx, step, is_noisy, b0, W, H, C, nb, latent, nullptr, 1.0f); }
    void blend_mask(float* denoised) const {
        if (p->denoise_mask && p->init_latent) {  // inpainting: denoised * mask + init_latent * (1 - mask), the mask broadcast over channels and images (stable-diffusion.cpp:2888-2890)
            const size_t plane = (size_t)W * H;
            for (int b = 0; b < nb; ++b)
                for (int c = 0; c < C; ++c) {
                    float* d        = denoised + (size_t)b * per + (size_t)c * plane;
                    const float* il = p->init_latent + (size_t)c * plane;
                    for (size_t k = 0; k < plane; ++k) {
                        const float m = p->denoise_mask[k];
                        d[k]          = d[k] * m + il[k] * (1.0f - m);
                    }
                }
        }
    }
};
// img2img (stable-diffusion.cpp:4924-4980): with an init latent and strength < 1 the trajectory starts t_enc = steps * strength steps before the end of the ladder
static std::vector<float> call_sigmas(sdm_ctx_t* ctx, const sdm_img_gen_params_t* p, int image_seq_len, int scheduler) {
    // set_flow_shift (stable-diffusion.cpp:3106-3115): the request's shift, or the family default (SD3.x 3.0, FLUX.1-dev 1.15), on the flow denoisers
    const float fs = p->sample_params.flow_shift;
    ctx->flow_denoiser.shift = (std::isfinite(fs) && fs > 0.f) ? fs : 3.0f;
    ctx->flux_denoiser.shift = (std::isfinite(fs) && fs > 0.f) ? fs : 1.15f;
    // custom sigmas replace the scheduler's ladder as they are (stable-diffusion.cpp:4337-4349)
    std::vector<float> sigmas = (p->sample_params.custom_sigmas && p->sample_params.custom_sigmas_count > 1)
                                    ? std::vector<float>(p->sample_params.custom_sigmas, p->sample_params.custom_sigmas + p->sample_params.custom_sigmas_count)
                                    : ctx->get_sigmas(p->sample_params.sample_steps, image_seq_len, scheduler);
    if (p->init_latent && p->strength < 1.f && !sigmas.empty()) {
        // (custom sigmas set sample_steps to their count - 1 first, stable-diffusion.cpp:4337-4345; a scheduler that returned fewer sigmas than steps + 1 — beta — likewise here)
        const int sample_steps = std::min(p->sample_params.sample_steps, (int)sigmas.size() - 1) < p->sample_params.sample_steps || p->sample_params.custom_sigmas_count > 1
                                     ? (int)sigmas.size() - 1
                                     : p->sample_params.sample_steps;
        size_t t_enc           = static_cast<size_t>(sample_steps * p->strength);
        if (t_enc == static_cast<size_t>(sample_steps)) t_enc--;
        const int64_t first = (int64_t)sample_steps - (int64_t)t_enc - 1;
        if (first > 0 && first < (int64_t)sigmas.size()) sigmas.erase(sigmas.begin(), sigmas.begin() + first);  // (a ladder shorter than steps + 1 — beta scheduler — keeps at least its last pair)
    }
    return sigmas;
}
// Denoiser::noise_scaling (denoiser.hpp:1181-1186 CompVis: latent + noise * sigma; :1274-1279 flow: latent * (1 - sigma) + noise * sigma); latent NULL = zeros (txt2img)
static inline void noise_scaling(float* x, const float* noise, const float* latent, size_t n, float sigma, bool flow) {
    if (!latent) {
        for (size_t i = 0; i < n; ++i) x[i] = 0.0f + noise[i] * sigma;
    } else if (flow) {
        const float om = 1.0f - sigma;
        for (size_t i = 0; i < n; ++i) x[i] = latent[i] * om + noise[i] * sigma;
    } else {
        for (size_t i = 0; i < n; ++i) x[i] = latent[i] + noise[i] * sigma;
    }
}
static bool sample_group(sdm_ctx_t* ctx, const sdm_img_gen_params_t* p, int b0, int nb, float* out) {
    const int W = p->width / 8, H = p->height / 8, C = ctx->latent_channels();
    const size_t per = (size_t)W * H * C;
    const sdm_sample_params_t& sp = p->sample_params;
    int method, scheduler;
    float eta;
    if (!resolve_sampling(ctx, sp, method, scheduler, eta)) return false;
    const std::vector<float> sigmas = call_sigmas(ctx, p, W * H, scheduler);  // image_seq_len = latent pixels (stable-diffusion.cpp:2983-2986)
    const int steps                 = (int)sigmas.size() - 1;
    if (steps < 1) {
        set_error("the scheduler returned no sigma ladder for " + std::to_string(sp.sample_steps) + " steps");
        return false;
    }

    // per-image RNG: seed+b; initial noise consumes offset 0 (stable-diffusion.cpp:5678-5683; rng == sampler_rng :886-889)
    std::vector<PhiloxRNG> rngs;
    std::vector<float> x(per * nb);
    for (int b = 0; b < nb; ++b) rngs.emplace_back((uint64_t)(p->seed + b0 + b));
    parallel_chunks((size_t)nb, [&](size_t i0, size_t i1) {
        for (size_t b = i0; b < i1; ++b) {
            std::vector<float> noise = rngs[b].randn((uint32_t)per);
            noise_scaling(&x[b * per], noise.data(), p->init_latent, per, sigmas[0], ctx->is_dit);
        }
    }, 2);
    HostDenoise denoise(ctx, p, W, H, C, nb, b0);
    denoise.n_sigmas = (int)sigmas.size();
    denoise.b0       = b0;
    ctx->step_cache_begin_trajectory(sigmas, method);  // init_sample_cache_runtime per sample() call, stable-diffusion.cpp:2578
    denoise.sc = &ctx->step_cache;
    std::vector<float> denoised(per * nb);
    std::vector<std::vector<float>> step_noise(nb);

    if (method != SDM_EULER_SAMPLE_METHOD && method != SDM_EULER_A_SAMPLE_METHOD) {
        // the multi-stage / multi-step samplers (sampler.hpp: run_sampler_generic): per-image Philox streams, one draw of `per` normals per image and request
        const bool ok = run_sampler_generic(method, [&](const float* xin, float sigma, float* den, float* unc, int step) { return denoise(xin, sigma, den, unc, step); }, x, sigmas,
                                            [&](float* dst) {
                                                for (int b = 0; b < nb; ++b) {
                                                    const std::vector<float> nz = rngs[b].randn((uint32_t)per);
                                                    memcpy(dst + (size_t)b * per, nz.data(), per * sizeof(float));
                                                }
                                            },
                                            eta, ctx->is_dit, nb,
                                            [&](int b, uint32_t cnt, float* dst) {
                                                const std::vector<float> nz = rngs[b].randn(cnt);
                                                memcpy(dst, nz.data(), cnt * sizeof(float));
                                            });
        if (!ok) return false;
        memcpy(out, x.data(), x.size() * sizeof(float));
        return true;
    }

    for (int i = 0; i < steps; ++i) {
        const float sigma = sigmas[i], sigma_to = sigmas[i + 1];
        // The ancestral noise of this step depends on the sigma ladder only, not on the model output: draw it (host Philox, 0.7 ms per
        // SD1.5 image) on a helper thread WHILE the device runs the forward, instead of after it.  Same per-image streams, same order.
        float sigma_down = 0.f, sigma_up = 0.f, alpha_scale = 1.f;
        std::future<void> noise_job;
        if (method == SDM_EULER_A_SAMPLE_METHOD && sigma_to != 0.f && eta != 0.f) {
            if (ctx->is_dit)  // flow denoisers (SD3.5, FLUX): get_ancestral_step(..., is_flow_denoiser), denoiser.hpp:1501-1511
                ancestral_step_flow(sigma, sigma_to, eta, sigma_down, sigma_up, alpha_scale);
            else
                ancestral_step(sigma, sigma_to, eta, sigma_down, sigma_up);
            if (sigma_up > 0.f)
                noise_job = std::async(std::launch::async, [&]() {
                    for (int b = 0; b < nb; ++b) step_noise[b] = rngs[b].randn((uint32_t)per);
                });
        }
        struct JoinNoise {  // an early return must not leave the helper writing into dead stack frames
            std::future<void>& f;
            ~JoinNoise() {
                if (f.valid()) f.wait();
            }
        } join_noise{noise_job};
        if (!denoise(x.data(), sigma, denoised.data(), nullptr, i + 1)) return false;
        // the update itself: sample_euler_ancestral / sample_euler (sampler.hpp: sampler_update — the function tests hold bit-for-bit against the reference's
        // own src/runtime/denoiser.hpp compiled into oracle/_ref)
        sampler_update(x.data(), denoised.data(), per, nb, method == SDM_EULER_A_SAMPLE_METHOD, ctx->is_dit, sigma, sigma_to, eta, sigma_down, sigma_up, alpha_scale,
                       [&](int b) -> const float* {
                           if (noise_job.valid()) noise_job.get();
                           return step_noise[b].data();
                       });
    }
    memcpy(out, x.data(), x.size() * sizeof(float));
    return true;
}

// The step caches' two device passes (include/ggml-mi355x.h) as the device-resident sampler and sd_step_cache_kernels reach them: plug-in exports found through the
// registry's get_proc_address like ggml_backend_mi355x_get_stream, enqueued on the backend's stream between two graphs.  A backend without them (the CPU oracle of
// the tests) gets the same quantities from the host: the tensors are read back, the sums formed like the host loop's (one float, sequential) and written back.
struct StepCacheDevice {
    typedef bool (*probe_fn)(ggml_backend_t, const float*, float, const float*, int64_t, float*);
    typedef bool (*record_fn)(ggml_backend_t, const float*, const float*, float*, float*, float*, int64_t, int, int64_t, bool, float*);
    ggml_backend_t backend = nullptr;
    // the CacheDIT modes' probe, Spectrum's forecast and the push of a computed `denoised` into its ring slot (a device-to-device copy enqueued on the backend stream)
    typedef bool (*predict_fn)(ggml_backend_t, const float*, int64_t, const int*, int, const float*, float, int64_t, float*);
    typedef bool (*push_fn)(ggml_backend_t, const float*, float*, int64_t);
    probe_fn probe_k       = nullptr;
    record_fn record_k     = nullptr;
    probe_fn probe_rel_k   = nullptr;
    predict_fn predict_k   = nullptr;
    push_fn push_k         = nullptr;
    bool exports_missing   = false;
    bool mode_exports_missing = false;  // ... of the three above (an MI355X plug-in older than these modes)
    std::vector<float> a, b, c, d;
    explicit StepCacheDevice(ggml_backend_t be) : backend(be) {
        ggml_backend_dev_t dev = ggml_backend_get_device(be);
        ggml_backend_reg_t reg = dev ? ggml_backend_dev_backend_reg(dev) : nullptr;
        if (reg) {
            probe_k  = (probe_fn)ggml_backend_reg_get_proc_address(reg, "ggml_backend_mi355x_step_cache_probe");
            record_k = (record_fn)ggml_backend_reg_get_proc_address(reg, "ggml_backend_mi355x_step_cache_record");
        }
        if (reg) {
            probe_rel_k = (probe_fn)ggml_backend_reg_get_proc_address(reg, "ggml_backend_mi355x_step_cache_probe_rel");
            predict_k   = (predict_fn)ggml_backend_reg_get_proc_address(reg, "ggml_backend_mi355x_spectrum_predict");
            push_k      = (push_fn)ggml_backend_reg_get_proc_address(reg, "ggml_backend_mi355x_spectrum_push");
        }
        if (!probe_k || !record_k) probe_k = nullptr, record_k = nullptr;
        if (!probe_k || !probe_rel_k || !predict_k || !push_k) probe_rel_k = nullptr, predict_k = nullptr, push_k = nullptr;
        mode_exports_missing = !probe_rel_k && reg && strcmp(ggml_backend_reg_name(reg), "MI355X") == 0;
        // the product backend without its passes is an error, never a quiet fall-back to full-tensor read-backs; any other backend takes the host restatement
        exports_missing = !probe_k && reg && strcmp(ggml_backend_reg_name(reg), "MI355X") == 0;
    }
    bool on_device() const { return probe_k != nullptr; }
    // stats[0] = sum |x * c_in - prev_in| over n floats
    bool probe(ggml_tensor* x, float c_in, ggml_tensor* prev_in, int64_t n, ggml_tensor* stats) {
        if (probe_k) return probe_k(backend, (const float*)x->data, c_in, (const float*)prev_in->data, n, (float*)stats->data);
        a.resize((size_t)n), b.resize((size_t)n);
        ggml_backend_tensor_get(x, a.data(), 0, (size_t)n * sizeof(float));
        ggml_backend_tensor_get(prev_in, b.data(), 0, (size_t)n * sizeof(float));
        float sum = 0.0f;
        for (int64_t i = 0; i < n; ++i) {
            const float m = a[(size_t)i] * c_in;
            sum += std::fabs(m - b[(size_t)i]);
        }
        ggml_backend_tensor_set(stats, &sum, 0, sizeof(float));
        return true;
    }
    // stats[0] = sum |x * c_in - prev_in|, stats[3] = sum |prev_in| over n floats (calculate_residual_diff's two sums)
    bool probe_rel(ggml_tensor* x, float c_in, ggml_tensor* prev_in, int64_t n, ggml_tensor* stats) {
        if (probe_rel_k) return probe_rel_k(backend, (const float*)x->data, c_in, (const float*)prev_in->data, n, (float*)stats->data);
        a.resize((size_t)n), b.resize((size_t)n);
        ggml_backend_tensor_get(x, a.data(), 0, (size_t)n * sizeof(float));
        ggml_backend_tensor_get(prev_in, b.data(), 0, (size_t)n * sizeof(float));
        float sum = 0.0f, mag = 0.0f;
        for (int64_t i = 0; i < n; ++i) {
            const float m = a[(size_t)i] * c_in;
            sum += std::fabs(b[(size_t)i] - m);
            mag += std::fabs(b[(size_t)i]);
        }
        ggml_backend_tensor_set(stats, &sum, 0, sizeof(float));
        ggml_backend_tensor_set(stats, &mag, 3 * sizeof(float), sizeof(float));
        return true;
    }
    // Spectrum: ring [stride, K] f32, out n floats; order / weights: k host values, oldest first
    bool spectrum_predict(ggml_tensor* ring, int64_t stride, int K, const int* order, int k, const float* weights, float w, int64_t n, ggml_tensor* out) {
        if (predict_k) return predict_k(backend, (const float*)ring->data, stride, order, k, weights, w, n, (float*)out->data);
        a.resize((size_t)(stride * K)), b.resize((size_t)n);
        ggml_backend_tensor_get(ring, a.data(), 0, a.size() * sizeof(float));
        spectrum_predict_host(a.data(), (size_t)stride, order, k, weights, w, (size_t)n, b.data());
        ggml_backend_tensor_set(out, b.data(), 0, (size_t)n * sizeof(float));
        return true;
    }
    bool spectrum_push(ggml_tensor* src, ggml_tensor* ring, int64_t stride, int slot, int64_t n) {
        if (push_k) return push_k(backend, (const float*)src->data, (float*)ring->data + (int64_t)slot * stride, n);
        a.resize((size_t)n);
        ggml_backend_tensor_get(src, a.data(), 0, (size_t)n * sizeof(float));
        ggml_backend_tensor_set(ring, a.data(), (size_t)slot * (size_t)stride * sizeof(float), (size_t)n * sizeof(float));
        return true;
    }
    // in / prev_in / prev_out [per, nb], out / diff [per, k, nb]: the stored differences, the anchor's previous input / output, stats[1] and stats[2]
    bool record(ggml_tensor* in, ggml_tensor* out, ggml_tensor* prev_in, ggml_tensor* prev_out, ggml_tensor* diff, int64_t per, int k, int64_t nb, bool has_prev_out,
                ggml_tensor* stats) {
        if (record_k)
            return record_k(backend, (const float*)in->data, (const float*)out->data, (float*)prev_in->data, (float*)prev_out->data, (float*)diff->data, per, k, nb, has_prev_out,
                            (float*)stats->data);
        const size_t n = (size_t)(per * nb);
        a.resize(n), b.resize(n * k), c.resize(n), d.resize(n * k);
        ggml_backend_tensor_get(in, a.data(), 0, n * sizeof(float));
        ggml_backend_tensor_get(out, b.data(), 0, n * k * sizeof(float));
        if (has_prev_out) ggml_backend_tensor_get(prev_out, c.data(), 0, n * sizeof(float));
        float sums[2] = {0.0f, 0.0f};
        for (int64_t im = 0; im < nb; ++im)
            for (int64_t i = 0; i < per; ++i) {
                const size_t e = (size_t)(im * per + i), o = (size_t)(im * k * per + i);
                for (int j = 0; j < k; ++j) d[o + (size_t)j * per] = b[o + (size_t)j * per] - a[e];
                if (has_prev_out) sums[0] += std::fabs(b[o] - c[e]);
                sums[1] += std::fabs(b[o]);
                c[e] = b[o];
            }
        ggml_backend_tensor_set(diff, d.data(), 0, n * k * sizeof(float));
        ggml_backend_tensor_set(prev_in, a.data(), 0, n * sizeof(float));
        ggml_backend_tensor_set(prev_out, c.data(), 0, n * sizeof(float));
        ggml_backend_tensor_set(stats, sums, sizeof(float), sizeof(sums));
        return true;
    }
};

// ---- device-resident sampler -----------------------------------------------------------------------
// The reference crosses the host boundary three times per model call (x*c_in up, eps down, CFG / Euler on the host:
// stable-diffusion.cpp:2636-2664, 2855-2896; denoiser.hpp:1513-1546).  Here one graph per step carries the whole iteration —
//   x*c_in -> (cond, uncond interleaved) model call -> uncond + s*(cond - uncond) -> *c_out + x*c_skip -> Euler(-A) update (+ noise*sigma_up)
//   -> CPY back into the persistent latent tensor
// — on nodes the backend already runs (MUL / SUB / ADD / DIV with a 1-element broadcast operand, REPEAT, CPY), and every step's
// scalars arrive as ONE 8-float input, so all steps share one cached plan.  Nothing is read back until the last step: uploads and
// graphs are queued on the backend stream (set_tensor_async / graph_compute_async) and the host builds step k+1 while step k runs.
// Ancestral noise stays the host Philox stream (bit-reproducible, rng_philox.hpp:101-122), uploaded per step (64 KB per SD1.5 image).
//
// Step cache (sd_set_step_cache): the decision depends on data, so an ACTIVE step cannot be queued blindly.  Per active step: the probe pass sums |x * c_in - prev_in|
// from the live latents, ONE 16-byte read-back of cache.stats synchronises and delivers that sum together with the two the previous computed step's record pass left
// there, the host state machine (step_cache.hpp) decides; a computed step runs the RECORDING variant of the step graph (noised and eps pass through cache.in /
// cache.out on their way) followed by the record pass, a skipped step the SKIP-STEP graph (eps_j = noised + diff_j, then the same combine and update).  Inactive
// steps, and every trajectory without an armed cache, use the plain step graph under its unchanged signature.  Active steps give up the build-ahead overlap.
// The CacheDIT modes take the same flow with the probe_rel pass (two sums) in place of the probe; their record pass is the same one, its two sums unused.
//
// Spectrum: the schedule depends on counters only, so nothing is read back and the build-ahead overlap stays.  A computed call runs the SPECTRUM-RECORDING variant of
// the step graph (denoised passes through spectrum.denoised on its way into the update) followed by a device-to-device copy into the call's ring slot, enqueued on
// the backend stream; a predicted call enqueues the forecast pass (kernels/step_cache.hip) into spectrum.denoised — the host has the weights: they depend on taus
// only — and then the PREDICTED-STEP graph, the tail of the step graph from `denoised` on.  Calls from the stop call on feed nothing any more: plain step graph.
static bool sample_group_device(sdm_ctx_t* ctx, const sdm_img_gen_params_t* p, int b0, int nb, float* out, bool* handled) {
    *handled = false;
    const int W = p->width / 8, H = p->height / 8, C = ctx->latent_channels();
    const sdm_sample_params_t& sp = p->sample_params;
    const GuidancePlan gp = resolve_guidance_plan(ctx, p);  // (a plain context: use_uncond = txt_cfg != 1 with an uncond conditioning, no third branch)
    const bool use_cfg = gp.use_uncond;
    const bool has_y   = p->cond.c_vector != nullptr;
    if (gp.branches() > 1 && (p->cond.ctx_dim != p->uncond.ctx_dim || p->cond.n_tokens != p->uncond.n_tokens || has_y != (p->uncond.c_vector != nullptr))) return true;
    if (ctx->out_channels() != C) return true;  // learned-sigma heads are not sampled this way
    int method, scheduler;
    float eta;
    if (!resolve_sampling(ctx, sp, method, scheduler, eta)) {
        *handled = true;  // (the error is set: the host loop would refuse the same parameters)
        return false;
    }
    if (method != SDM_EULER_SAMPLE_METHOD && method != SDM_EULER_A_SAMPLE_METHOD) return true;  // multi-stage / multi-step samplers: the host loop around the device forward
    if (p->denoise_mask && p->init_latent) return true;  // the inpainting blend lives in the host loop's denoise call
    if (ApgParams{sp.apg_eta, sp.apg_momentum, sp.apg_norm_threshold, sp.apg_norm_threshold_smoothing}.enabled()) return true;  // adaptive projected guidance: norms and a momentum buffer on the host
    if (sp.slg_scale != 0.0f && sp.slg_layers && sp.slg_layer_count > 0 && ctx->is_dit && !ctx->is_flux) return true;  // skip-layer guidance: a third forward inside a step window
    *handled = true;
    const size_t per = (size_t)W * H * C;
    const std::vector<float> sigmas = call_sigmas(ctx, p, W * H, scheduler);
    const int steps                 = (int)sigmas.size() - 1;
    if (steps < 1) {
        set_error("the scheduler returned no sigma ladder for " + std::to_string(sp.sample_steps) + " steps");
        return false;
    }
    const bool euler_a              = method == SDM_EULER_A_SAMPLE_METHOD;
    const bool flow                 = ctx->is_dit;  // flow denoiser: ancestral steps rescale x by alpha_scale before the noise (denoiser.hpp:1536-1541)

    if (!ctx->sstate || ctx->sstate->W != W || ctx->sstate->H != H || ctx->sstate->C != C || ctx->sstate->N != nb) {
        ctx->sstate.reset(new sdm_ctx_t::SamplerState());
        auto& st = *ctx->sstate;
        ggml_init_params ip{0, nullptr, true};
        st.sctx  = ggml_init(ip);
        st.x     = ggml_new_tensor_4d(st.sctx, GGML_TYPE_F32, W, H, C, nb);
        st.noise = ggml_new_tensor_4d(st.sctx, GGML_TYPE_F32, W, H, C, nb);
        st.eps   = ggml_new_tensor_4d(st.sctx, GGML_TYPE_F32, W, H, C, nb);  // CFG-pair split: this rank's weighted eps, summed in place by the exchange
        ggml_set_name(st.eps, "sampler.eps");
        ggml_set_name(st.x, "sampler.x");
        ggml_set_name(st.noise, "sampler.noise");
        st.buf = ggml_backend_alloc_ctx_tensors(st.sctx, ctx->backend);
        if (!st.buf) {
            ctx->sstate.reset();
            set_error("sampler state allocation failed");
            return false;
        }
        st.W = W, st.H = H, st.C = C, st.N = nb;
    }
    auto& st = *ctx->sstate;

    std::vector<PhiloxRNG> rngs;
    std::vector<float> x(per * nb), noise(per * nb, 0.f);
    for (int b = 0; b < nb; ++b) rngs.emplace_back((uint64_t)(p->seed + b0 + b));
    // one independent Philox stream per image (seed + b): the images' draws run on separate host threads (0.7 ms per SD1.5 image each)
    parallel_chunks((size_t)nb, [&](size_t i0, size_t i1) {
        for (size_t b = i0; b < i1; ++b) {
            std::vector<float> nz = rngs[b].randn((uint32_t)per);
            noise_scaling(&x[b * per], nz.data(), p->init_latent, per, sigmas[0], ctx->is_dit);
        }
    }, 2);
    ggml_backend_tensor_set_async(ctx->backend, st.x, x.data(), 0, x.size() * sizeof(float));
    ggml_backend_tensor_set_async(ctx->backend, st.noise, noise.data(), 0, noise.size() * sizeof(float));

    // CFG-pair split (guidance.cpp:149-179 computed on two GPUs): this context runs ONE branch per step and writes
    // weight * eps (weight = s on the cond rank, 1 - s on the uncond rank) to st.eps; the caller's exchange sums the two ranks' buffers in
    // place, in HBM, ordered on the backend stream; a second small graph takes the Euler(-A) update from the sum.  Both ranks then hold the
    // same latents (same Philox streams), so nothing else is exchanged.
    const bool pair = ctx->pair_fn != nullptr && use_cfg;
    // conditioning of the (cond, uncond) pair, tiled over the images by the model graph's own ggml_repeat
    // K evaluations per image in the step graph: cond [, uncond] [, img_uncond — uncond's text with the img_uncond concat]; two of them combine as
    // second + s * (cond - second) whichever the second is (guidance.cpp:171, 175), three as the three-term form (:166-168)
    const int K       = pair ? 1 : gp.branches();
    const bool both   = K == 2;
    const bool three  = K == 3;
    const int n_model = K * nb;
    const int ctx_n   = K;
    const size_t cn   = (size_t)p->cond.ctx_dim * p->cond.n_tokens;
    const sd_condition_t& first = (pair && ctx->pair_branch == 1) ? p->uncond : p->cond;
    std::vector<float> c2(cn * ctx_n), y2;
    memcpy(&c2[0], first.c_crossattn, cn * sizeof(float));
    for (int j = 1; j < K; ++j) memcpy(&c2[cn * j], p->uncond.c_crossattn, cn * sizeof(float));
    if (has_y) {
        y2.resize((size_t)p->cond.vector_dim * ctx_n);
        memcpy(&y2[0], first.c_vector, p->cond.vector_dim * sizeof(float));
        for (int j = 1; j < K; ++j) memcpy(&y2[(size_t)p->cond.vector_dim * j], p->uncond.c_vector, p->cond.vector_dim * sizeof(float));
    }
    // c_concat (inpaint / pix2pix UNets): resident for the trajectory, uploaded once — [W,H,cc,K] when the batch shares it (row j is branch j's: `concat` for cond and
    // uncond, `img_uncond_concat` on the img_uncond seat; the model graph's REPEAT tiles it over the images) or [W,H,cc,K*nb] per image, in the order of the model batch
    // image tokens (sd_set_ip_adapter): one [ip_dim, n_ip, K] input, row j is branch j's — assembled once per trajectory, tiled over the images like the context
    const bool ip_on             = !ctx->is_dit && ctx->ip_active();
    const std::vector<float> ip2 = ip_on ? ctx->ip_rows(K, pair && ctx->pair_branch == 1) : std::vector<float>();
    const float *cat_host = nullptr, *cat_img_host = nullptr;
    int cat_cc = 0, cat_n = 0;
    group_concat(ctx, b0, nb, cat_host, cat_img_host, cat_cc, cat_n);
    std::vector<float> cat_stage;
    ggml_tensor* cat_dev = nullptr;
    if (cat_host) {
        const int rows     = cat_n == 1 ? 1 : nb;
        const size_t ccper = (size_t)W * H * cat_cc;
        const int img_seat = (gp.use_img_uncond && !pair) ? K - 1 : -1;
        if (!st.concat || st.concat->t->ne[2] != cat_cc || st.concat->t->ne[3] != (int64_t)K * rows) {
            st.concat.reset(new sdm_ctx_t::SamplerState::Concat());
            auto& sc_ = *st.concat;
            ggml_init_params ip{0, nullptr, true};
            sc_.cctx = ggml_init(ip);
            sc_.t    = ggml_new_tensor_4d(sc_.cctx, GGML_TYPE_F32, W, H, cat_cc, (int64_t)K * rows);
            ggml_set_name(sc_.t, "sampler.concat");
            sc_.buf = ggml_backend_alloc_ctx_tensors(sc_.cctx, ctx->backend);
            if (!sc_.buf) {
                st.concat.reset();
                set_error("sampler concat state allocation failed");
                return false;
            }
            static std::atomic<uint64_t> g_concat_serial{0};
            sc_.serial = ++g_concat_serial;
        }
        cat_stage.resize((size_t)K * rows * ccper);
        for (int b = 0; b < rows; ++b)
            for (int j = 0; j < K; ++j)
                memcpy(&cat_stage[((size_t)b * K + j) * ccper], (j == img_seat ? cat_img_host : cat_host) + (size_t)b * ccper, ccper * sizeof(float));
        cat_dev = st.concat->t;
        ggml_backend_tensor_set_async(ctx->backend, cat_dev, cat_stage.data(), 0, cat_stage.size() * sizeof(float));
    }
    void* pair_stream = nullptr;
    if (pair) {
        typedef void* (*get_stream_fn)(ggml_backend_t);
        ggml_backend_dev_t dev = ggml_backend_get_device(ctx->backend);
        ggml_backend_reg_t reg = dev ? ggml_backend_dev_backend_reg(dev) : nullptr;
        get_stream_fn gs       = reg ? (get_stream_fn)ggml_backend_reg_get_proc_address(reg, "ggml_backend_mi355x_get_stream") : nullptr;
        pair_stream            = gs ? gs(ctx->backend) : nullptr;  // host backends (the CPU oracle in the tests): no stream, calls are synchronous
    }
    ctx->step_cache_begin_trajectory(sigmas, method);
    StepCacheRuntime& rt = ctx->step_cache;
    const int ck = both ? 2 : 1;  // conditions per image in the step graph's eps
    StepCacheDevice cache_dev(ctx->backend);
    if ((rt.is_cachedit() || rt.spectrum_enabled) && cache_dev.mode_exports_missing) {
        set_error("step cache: the MI355X backend does not export the passes of this mode (ggml_backend_mi355x_step_cache_probe_rel / _spectrum_predict / _spectrum_push)");
        return false;
    }
    if (rt.spectrum_enabled) {
        const int K = rt.spectrum.K;
        if (!st.spectrum || st.spectrum->K != K) {
            st.spectrum.reset(new sdm_ctx_t::SamplerState::Spectrum());
            auto& ss = *st.spectrum;
            ggml_init_params ip{0, nullptr, true};
            ss.cctx     = ggml_init(ip);
            ss.stride   = ((int64_t)(per * (size_t)nb) + 3) / 4 * 4;
            ss.ring     = ggml_new_tensor_2d(ss.cctx, GGML_TYPE_F32, ss.stride, K);
            ss.denoised = ggml_new_tensor_4d(ss.cctx, GGML_TYPE_F32, W, H, C, nb);
            ggml_set_name(ss.ring, "spectrum.ring");
            ggml_set_name(ss.denoised, "spectrum.denoised");
            ss.buf = ggml_backend_alloc_ctx_tensors(ss.cctx, ctx->backend);
            if (!ss.buf) {
                st.spectrum.reset();
                set_error("step cache state allocation failed");
                return false;
            }
            ss.K = K;
            static std::atomic<uint64_t> g_spectrum_serial{0};
            ss.serial = ++g_spectrum_serial;
        }
    }
    sdm_ctx_t::SamplerState::Spectrum* ss = rt.spectrum_enabled ? st.spectrum.get() : nullptr;
    if (rt.armed()) {  // (never together with a split CFG pair: sd_sample_latents refuses that)
        if (cache_dev.exports_missing) {
            set_error("step cache: the MI355X backend does not export its step-cache passes (ggml_backend_mi355x_step_cache_probe / _record)");
            return false;
        }
        if (!st.cache || st.cache->k != ck) {
            st.cache.reset(new sdm_ctx_t::SamplerState::Cache());
            auto& cc = *st.cache;
            ggml_init_params ip{0, nullptr, true};
            cc.cctx     = ggml_init(ip);
            cc.in       = ggml_new_tensor_4d(cc.cctx, GGML_TYPE_F32, W, H, C, nb);
            cc.prev_in  = ggml_new_tensor_4d(cc.cctx, GGML_TYPE_F32, W, H, C, nb);
            cc.prev_out = ggml_new_tensor_4d(cc.cctx, GGML_TYPE_F32, W, H, C, nb);
            // the layout the step graph gives eps: cond and uncond of an image adjacent
            cc.out   = both ? ggml_new_tensor_3d(cc.cctx, GGML_TYPE_F32, (int64_t)((size_t)W * H * C), 2, nb) : ggml_new_tensor_4d(cc.cctx, GGML_TYPE_F32, W, H, C, nb);
            cc.diff  = both ? ggml_new_tensor_3d(cc.cctx, GGML_TYPE_F32, (int64_t)((size_t)W * H * C), 2, nb) : ggml_new_tensor_4d(cc.cctx, GGML_TYPE_F32, W, H, C, nb);
            cc.stats = ggml_new_tensor_1d(cc.cctx, GGML_TYPE_F32, 4);
            ggml_set_name(cc.in, "cache.in");
            ggml_set_name(cc.out, "cache.out");
            ggml_set_name(cc.prev_in, "cache.prev_in");
            ggml_set_name(cc.prev_out, "cache.prev_out");
            ggml_set_name(cc.diff, "cache.diff");
            ggml_set_name(cc.stats, "cache.stats");
            cc.buf = ggml_backend_alloc_ctx_tensors(cc.cctx, ctx->backend);
            if (!cc.buf) {
                st.cache.reset();
                set_error("step cache state allocation failed");
                return false;
            }
            cc.k = ck;
            static std::atomic<uint64_t> g_cache_serial{0};
            cc.serial = ++g_cache_serial;
        }
    }
    sdm_ctx_t::SamplerState::Cache* cc = rt.armed() ? st.cache.get() : nullptr;
    // latent previews: with a denoised preview installed, `denoised` of a due step passes through preview.denoised (like variant 3 passes it through
    // spectrum.denoised) and the byte stage reads it there behind the step graph; with none installed nothing below exists
    const PreviewState& pvs = ctx->preview;
    if (pvs.on() && pvs.denoised && !st.preview) {
        st.preview.reset(new sdm_ctx_t::SamplerState::Preview());
        auto& sp_ = *st.preview;
        ggml_init_params ip{0, nullptr, true};
        sp_.cctx     = ggml_init(ip);
        sp_.denoised = ggml_new_tensor_4d(sp_.cctx, GGML_TYPE_F32, W, H, C, nb);
        ggml_set_name(sp_.denoised, "preview.denoised");
        sp_.buf = ggml_backend_alloc_ctx_tensors(sp_.cctx, ctx->backend);
        if (!sp_.buf) {
            st.preview.reset();
            set_error("preview state allocation failed");
            return false;
        }
        static std::atomic<uint64_t> g_preview_serial{0};
        sp_.serial = ++g_preview_serial;
        sp_.step_runner.backend = sp_.skip_runner.backend = ctx->backend;
        sp_.step_runner.graph_size = ctx->unet_runner.graph_size;
        sp_.skip_runner.graph_size = ctx->skip_runner.graph_size;
    }
    sdm_ctx_t::SamplerState::Preview* pvt = (pvs.on() && pvs.denoised) ? st.preview.get() : nullptr;
    const std::string preview_tag         = pvt ? " preview" + std::to_string(pvt->serial) : std::string();
    int pending = -1;  // trace record of the computed step whose record-pass sums have not been read back yet
    auto book_pending = [&](const float* stats) {  // after_condition of that step: cond, then uncond (which only marks its difference as stored)
        sdm_cache_step_t* rec = &rt.trace[(size_t)pending];
        const float ne        = static_cast<float>(per * (size_t)nb);
        rt.after_condition(0, stats[1] / ne, stats[2] / ne, rec);
        if (ck == 2) rt.after_condition(1, 0.0f, 0.0f, rec);
        pending = -1;
    };
    ModelSideInputs si;
    if (!prepare_side_inputs(ctx, W, H, n_model, p->cond.n_tokens, has_y, si)) return false;
    std::vector<float> ts(n_model);
    Runner& r = ctx->unet_runner;
    char step_sig[360];  // every step of the trajectory replays ONE cached graph: only the 8 scalars, the timesteps and the conditioning are re-uploaded
    int sig_n = snprintf(step_sig, sizeof(step_sig), "step %d %d %d %d cfg%d ea%d %lld %lld y%lld %p pair%d", W, H, C, nb, (int)use_cfg, (int)euler_a + 2 * (int)flow,
                         (long long)p->cond.ctx_dim, (long long)p->cond.n_tokens, (long long)(has_y ? p->cond.vector_dim : -1), (void*)st.x, (int)pair);
    if (cat_dev)  // graphs with a concat input: its width, the branches per image, whether the last seat is img_uncond's, and the resident tensor they name
        snprintf(step_sig + sig_n, sizeof(step_sig) - (size_t)sig_n, " cc%d K%d iu%d pi%d concat%llu", cat_cc, K, (int)gp.use_img_uncond, (int)(cat_n != 1),
                 (unsigned long long)st.concat->serial);
    const std::string update_sig = std::string("update ") + step_sig;
    if (ip_on) {  // graphs with image tokens: their count and the strength (a node parameter); the tokens themselves are an input
        const size_t at = strlen(step_sig);
        snprintf(step_sig + at, sizeof(step_sig) - at, " ip%lld s%a", (long long)ctx->ip_set_n, (double)ctx->ip_strength);
    }
    const std::string cache_tag  = cc ? " cache" + std::to_string(cc->serial) : std::string();
    const std::string record_sig = std::string("record ") + step_sig + cache_tag;  // the recording variant and the skip-step graph: plans of their own
    const std::string skip_sig   = std::string("skip ") + step_sig + cache_tag;
    const std::string spectrum_tag        = ss ? " spectrum" + std::to_string(ss->serial) : std::string();
    const std::string spectrum_record_sig = std::string("spectrum-record ") + step_sig + spectrum_tag;
    const std::string spectrum_step_sig   = std::string("spectrum-step ") + step_sig + spectrum_tag;
    const bool rel = rt.is_cachedit();

    for (int i = 0; i < steps; ++i) {
        const float sigma = sigmas[i], sigma_to = sigmas[i + 1];
        float c_skip, c_out, c_in, t_model;
        step_scalings(ctx, sp, sigma, c_skip, c_out, c_in, t_model);
        std::fill(ts.begin(), ts.end(), t_model);
        // scalars of this step: {c_in, cfg scale, c_out, c_skip, a, b, noise gain, alpha}; Euler-A: x' = (a*x + b*denoised) [* alpha on flow models] + gain*noise;
        // Euler: x' = x + ((x - denoised) / a) * b with a = sigma, b = sigma_to - sigma
        // (a ninth scalar, img_cfg, exists only on graphs with a third branch: every other graph keeps its 8 scalars and its signature)
        float sc[9] = {c_in, pair ? (ctx->pair_branch == 0 ? sp.txt_cfg : 1.0f - sp.txt_cfg) : sp.txt_cfg, c_out, c_skip, 0.f, 0.f, 0.f, 1.f, gp.img_cfg};
        const int n_sc = three ? 9 : 8;
        bool fresh_noise = false;
        if (euler_a) {
            if (sigma_to == 0.f) {
                sc[4] = 0.f, sc[5] = 1.f;
            } else if (eta == 0.f) {
                const float ratio = sigma_to / sigma;
                sc[4] = ratio, sc[5] = (float)(1.0 - ratio);
            } else {
                float sigma_down, sigma_up, alpha_scale = 1.f;
                if (flow)
                    ancestral_step_flow(sigma, sigma_to, eta, sigma_down, sigma_up, alpha_scale);
                else
                    ancestral_step(sigma, sigma_to, eta, sigma_down, sigma_up);
                const float ratio = sigma_down / sigma;
                sc[4] = ratio, sc[5] = 1.0f - ratio;
                if (sigma_up > 0.f) {
                    sc[6]       = sigma_up;
                    sc[7]       = alpha_scale;
                    fresh_noise = true;
                }
            }
        } else {
            sc[4] = sigma, sc[5] = sigma_to - sigma;
        }
        if (fresh_noise) {
            parallel_chunks((size_t)nb, [&](size_t i0, size_t i1) {
                for (size_t b = i0; b < i1; ++b) {
                    std::vector<float> nz = rngs[b].randn((uint32_t)per);
                    memcpy(&noise[b * per], nz.data(), per * sizeof(float));
                }
            }, 2);
            ggml_backend_tensor_set_async(ctx->backend, st.noise, noise.data(), 0, noise.size() * sizeof(float));
        }
        // step cache: book the previous computed step, measure this step's input change, decide (see the note above the function)
        bool skip_step = false, record_step = false;
        if (cc) {
            const bool active  = rt.in_window(sigma);
            const bool measure = active && (pending >= 0 || rt.core().has_prev_input);  // once the pending record is booked the anchor has a previous input, output and difference
            float stats[4]     = {0.f, 0.f, 0.f, 0.f};
            if (measure && !(rel ? cache_dev.probe_rel(st.x, c_in, cc->prev_in, (int64_t)(per * (size_t)nb), cc->stats)
                                 : cache_dev.probe(st.x, c_in, cc->prev_in, (int64_t)(per * (size_t)nb), cc->stats))) {
                set_error("step cache: the probe pass could not be enqueued");
                return false;
            }
            if (measure || (pending >= 0 && !rel)) ggml_backend_tensor_get(cc->stats, stats, 0, sizeof(stats));  // THE synchronisation of an active step
            if (pending >= 0) book_pending(stats);  // (the CacheDIT modes book without numbers)
            rt.begin_call(i + 1, sigma);
            if (rt.step_is_active()) {
                if (rt.before_condition(0) == SC_MEASURE) skip_step = rel ? rt.decide_rel(stats[0], stats[3]) : rt.decide(stats[0] / static_cast<float>(per * (size_t)nb));
                record_step = !skip_step;
            }
        }
        // Spectrum: this call's record, and whether it is forecast; a computed call that can still feed a forecast records its denoised
        bool predict_step = false, spectrum_record = false;
        if (ss) {
            predict_step    = rt.spectrum_begin_call(i + 1, sigma);
            spectrum_record = !predict_step && !(rt.spectrum.stop_step > 0 && rt.spectrum.cnt >= rt.spectrum.stop_step);
        }
        const bool pv_den = pvt && pvs.wants(i + 1, false);  // this call's denoised is previewed: variants 0, 1 and 2 pass it through preview.denoised
        // variant 0: the step graph; 1: the same, recording (noised passes through cache.in, eps through cache.out); 2: the skip-step graph (no model call);
        // 3: the step graph with denoised passing through spectrum.denoised; 4: the predicted-step graph (denoised IS spectrum.denoised, no model call)
        auto build_variant = [&](int variant) {
          return [&, variant](GraphCtx& g, std::vector<HostInput>& in) {
            ggml_context* c  = g.ctx;
            ggml_tensor* tsc = ggml_new_tensor_1d(c, GGML_TYPE_F32, n_sc);
            ggml_set_input(tsc);
            in.push_back({tsc, sc, (size_t)n_sc * sizeof(float)});
            auto S = [&](int k) { return ggml_view_1d(c, tsc, 1, (size_t)k * sizeof(float)); };
            ggml_tensor* xs     = st.x;
            ggml_tensor* noised = variant == 4 ? nullptr : ggml_mul(c, xs, S(0));
            if (variant == 1) noised = ggml_cpy(c, noised, cc->in);
            ggml_tensor *eps = nullptr, *e3 = nullptr;  // e3: the pair's outputs [per, 2, nb], contiguous
            if (variant == 4) {  // no model input and no eps: denoised is already in spectrum.denoised
            } else if (variant == 2) {  // apply_condition_cache_diff for every condition: eps_j = noised + diff_j
                if (both) {
                    ggml_tensor* flat = ggml_reshape_3d(c, noised, (int64_t)per, 1, nb);
                    ggml_tensor* rep  = ggml_repeat(c, flat, ggml_new_tensor_3d(c, GGML_TYPE_F32, (int64_t)per, 2, nb));
                    e3                = ggml_add(c, rep, cc->diff);
                } else {
                    eps = ggml_add(c, noised, cc->diff);
                }
            } else {
                ggml_tensor* xin = noised;
                if (K > 1) {  // every image K times, its branches adjacent: [per, 1, nb] -> [per, K, nb]
                    ggml_tensor* flat = ggml_reshape_3d(c, noised, (int64_t)per, 1, nb);
                    ggml_tensor* rep  = ggml_repeat(c, flat, ggml_new_tensor_3d(c, GGML_TYPE_F32, (int64_t)per, K, nb));
                    xin               = ggml_reshape_4d(c, rep, W, H, C, K * nb);
                }
                // (cat_dev: the model's own graph appends it — [REPEAT over the images,] CONCAT along the channels, unet.hpp:554-559; with the chain above that is
                // the pattern the MI355X backend runs as one launch of k_model_input)
                eps = build_model_call(ctx, g, in, xin, n_model, ts.data(), c2.data(), p->cond.ctx_dim, p->cond.n_tokens, ctx_n,
                                       has_y ? y2.data() : nullptr, p->cond.vector_dim, ctx_n, si, cat_dev, ip_on ? ip2.data() : nullptr, ctx->ip_set_n, ctx_n, ctx->ip_strength);
                if (pair) return ggml_cpy(c, ggml_mul(c, eps, S(1)), st.eps);  // weight * eps of this rank's branch; the update follows the exchange
                if (K > 1) {
                    e3 = ggml_reshape_3d(c, ggml_cont(c, eps), (int64_t)per, K, nb);
                    if (variant == 1) e3 = ggml_cpy(c, e3, cc->out);
                } else if (variant == 1) {
                    eps = ggml_cpy(c, eps, cc->out);
                }
            }
            ggml_tensor* guided = eps;
            if (both && variant != 4) {  // uncond + s*(cond - uncond), guidance.cpp:171
                ggml_tensor* ec = ggml_view_3d(c, e3, (int64_t)per, 1, nb, e3->nb[1], e3->nb[2], 0);
                ggml_tensor* eu = ggml_view_3d(c, e3, (int64_t)per, 1, nb, e3->nb[1], e3->nb[2], e3->nb[1]);
                ggml_tensor* d  = ggml_mul(c, ggml_sub(c, ec, eu), S(1));
                guided          = ggml_reshape_4d(c, ggml_add(c, eu, d), W, H, C, nb);
            } else if (three && variant != 4) {  // iu + img * (u - iu) + txt * (c - u), guidance.cpp:166-168: six nodes, left to right (one launch of k_guidance3 on the MI355X backend)
                ggml_tensor* ec = ggml_view_3d(c, e3, (int64_t)per, 1, nb, e3->nb[1], e3->nb[2], 0);
                ggml_tensor* eu = ggml_view_3d(c, e3, (int64_t)per, 1, nb, e3->nb[1], e3->nb[2], e3->nb[1]);
                ggml_tensor* ei = ggml_view_3d(c, e3, (int64_t)per, 1, nb, e3->nb[1], e3->nb[2], 2 * e3->nb[1]);
                ggml_tensor* a1 = ggml_add(c, ei, ggml_mul(c, ggml_sub(c, eu, ei), S(8)));
                ggml_tensor* s2 = ggml_mul(c, ggml_sub(c, ec, eu), S(1));
                guided          = ggml_reshape_4d(c, ggml_add(c, a1, s2), W, H, C, nb);
            }
            ggml_tensor* den = variant == 4 ? ss->denoised : ggml_add(c, ggml_mul(c, guided, S(2)), ggml_mul(c, xs, S(3)));  // stable-diffusion.cpp:2876
            if (variant == 3) den = ggml_cpy(c, den, ss->denoised);
            if (pv_den && variant <= 2) den = ggml_cpy(c, den, pvt->denoised);
            ggml_tensor* xn;
            if (euler_a) {  // denoiser.hpp:1513-1546
                xn = ggml_add(c, ggml_mul(c, xs, S(4)), ggml_mul(c, den, S(5)));
                if (flow) xn = ggml_mul(c, xn, S(7));
                xn = ggml_add(c, xn, ggml_mul(c, st.noise, S(6)));
            } else {  // denoiser.hpp:1582-1597
                ggml_tensor* d = ggml_div(c, ggml_sub(c, xs, den), S(4));
                xn             = ggml_add(c, xs, ggml_mul(c, d, S(5)));
            }
            return ggml_cpy(c, xn, xs);
          };
        };
        std::vector<const void*> ptrs{sc, ts.data(), c2.data()};
        if (has_y) ptrs.push_back(y2.data());
        if (ip_on) ptrs.push_back(ip2.data());
        if (ctx->is_flux) {
            ptrs.push_back(si.guidance.data());
            ptrs.push_back(si.pe().data());
        }
        const std::string pv_tag = pv_den ? preview_tag : std::string();  // a capturing graph is a plan of its own; steps without a preview keep the signatures they had
        if (pvs.wants(i + 1, true) && !predict_step && !emit_preview(ctx, i + 1, true, b0, W, H, C, nb, nullptr, st.x, c_in)) return false;  // the model input, x * c_in
        if (skip_step) {
            if (!(pv_den ? pvt->skip_runner : ctx->skip_runner).compute(build_variant(2), nullptr, 0, skip_sig + pv_tag, {sc})) return false;
            if (pv_den && !emit_preview(ctx, i + 1, false, b0, W, H, C, nb, nullptr, pvt->denoised, 1.0f)) return false;
            continue;
        }
        if (predict_step) {
            float weights[SpectrumState::MAX_K];
            int order[SpectrumState::MAX_K];
            const int k = rt.spectrum.predict(weights, order);
            if (!cache_dev.spectrum_predict(ss->ring, ss->stride, ss->K, order, k, weights, rt.spectrum.config.w, (int64_t)(per * (size_t)nb), ss->denoised)) {
                set_error("step cache: the spectrum forecast pass could not be enqueued");
                return false;
            }
            if (!ctx->skip_runner.compute(build_variant(4), nullptr, 0, spectrum_step_sig, {sc})) return false;
            if (pv_den && !emit_preview(ctx, i + 1, false, b0, W, H, C, nb, nullptr, ss->denoised, 1.0f)) return false;  // the forecast
            continue;
        }
        const int variant = record_step ? 1 : (spectrum_record ? 3 : 0);  // (3 already has its denoised in spectrum.denoised: no capture, the signature it had)
        const bool capture = pv_den && variant != 3;
        if (!(capture ? pvt->step_runner : r).compute(build_variant(variant), nullptr, 0,
                                                      (record_step ? record_sig : (spectrum_record ? spectrum_record_sig : std::string(step_sig))) + (capture ? pv_tag : std::string()), ptrs))
            return false;
        if (capture) ++r.calls;  // (sd_stats_t::unet_calls counts the step graphs issued, whichever runner held them)
        if (ss) {  // SpectrumState::update: the counters, and — while a forecast can still follow — the tensor
            const int slot = rt.spectrum.update();
            if (spectrum_record && !cache_dev.spectrum_push(ss->denoised, ss->ring, ss->stride, slot, (int64_t)(per * (size_t)nb))) {
                set_error("step cache: the spectrum ring copy could not be enqueued");
                return false;
            }
        }
        if (record_step) {
            if (!cache_dev.record(cc->in, cc->out, cc->prev_in, cc->prev_out, cc->diff, (int64_t)per, ck, nb, rt.core().has_prev_output, cc->stats)) {
                set_error("step cache: the record pass could not be enqueued");
                return false;
            }
            pending = (int)rt.trace.size() - 1;
        }
        if (pv_den && !emit_preview(ctx, i + 1, false, b0, W, H, C, nb, nullptr, variant == 3 ? ss->denoised : pvt->denoised, 1.0f)) return false;
        if (pair) {
            if (!ctx->pair_fn(st.eps->data, (int64_t)(per * nb), pair_stream, ctx->pair_user)) {
                set_error("CFG-pair exchange failed");
                return false;
            }
            auto update = [&](GraphCtx& g, std::vector<HostInput>& in) {  // s*cond + (1-s)*uncond = uncond + s*(cond - uncond) is in st.eps
                ggml_context* c  = g.ctx;
                ggml_tensor* tsc = ggml_new_tensor_1d(c, GGML_TYPE_F32, 8);
                ggml_set_input(tsc);
                in.push_back({tsc, sc, 8 * sizeof(float)});
                auto S = [&](int k) { return ggml_view_1d(c, tsc, 1, (size_t)k * sizeof(float)); };
                ggml_tensor* xs  = st.x;
                ggml_tensor* den = ggml_add(c, ggml_mul(c, st.eps, S(2)), ggml_mul(c, xs, S(3)));
                ggml_tensor* xn;
                if (euler_a) {
                    xn = ggml_add(c, ggml_mul(c, xs, S(4)), ggml_mul(c, den, S(5)));
                    if (flow) xn = ggml_mul(c, xn, S(7));
                    xn = ggml_add(c, xn, ggml_mul(c, st.noise, S(6)));
                } else {
                    ggml_tensor* d = ggml_div(c, ggml_sub(c, xs, den), S(4));
                    xn             = ggml_add(c, xs, ggml_mul(c, d, S(5)));
                }
                return ggml_cpy(c, xn, xs);
            };
            if (!ctx->pair_runner.compute(update, nullptr, 0, update_sig, {sc})) return false;
        }
    }
    ggml_backend_tensor_get(st.x, out, 0, per * nb * sizeof(float));  // synchronises the stream
    if (pending >= 0) {  // the last computed step's sums, for the trace
        float stats[4];
        ggml_backend_tensor_get(cc->stats, stats, 0, sizeof(stats));
        book_pending(stats);
    }
    ctx->stats.unet_calls  = r.calls;
    ctx->stats.graph_nodes = r.last_nodes;
    if (r.galloc) ctx->stats.compute_buffer_bytes = ggml_gallocr_get_buffer_size(r.galloc, 0);
    return true;
}

// ---- step caches (csrc/host/step_cache.hpp) -----------------------------------------------------------------------------------
void sdm_cache_params_init(sdm_cache_params_t* p) { *p = sdm_cache_params_t{SDM_CACHE_DISABLED, INFINITY, 0.15f, 0.95f, 1.0f, true, true}; }  // sd_cache_params_init
bool sd_set_step_cache(sdm_ctx_t* ctx, const sdm_cache_params_t* params) {
    if (params && params->mode != SDM_CACHE_DISABLED &&
        (std::isnan(params->reuse_threshold) || std::isnan(params->start_percent) || std::isnan(params->end_percent) || std::isnan(params->error_decay_rate))) {
        set_error("sd_set_step_cache: NaN parameter");
        return false;
    }
    if (params)
        ctx->cache_params = *params;
    else
        sdm_cache_params_init(&ctx->cache_params);
    if (ctx->cache_params.mode == SDM_CACHE_DISABLED && ctx->sstate) ctx->sstate->cache.reset();
    if (ctx->cache_params.mode != SDM_CACHE_SPECTRUM && ctx->sstate) ctx->sstate->spectrum.reset();
    sdm_cache_dit_params_init(&ctx->cache_dit_params);  // (sd_set_step_cache_ex overwrites them afterwards)
    sdm_spectrum_params_init(&ctx->spectrum_params);
    return true;
}
void sdm_cache_dit_params_init(sdm_cache_dit_params_t* p) { *p = sdm_cache_dit_params_t{8, 0, 0.08f}; }                       // sd_cache_params_init, stable-diffusion.cpp:3514-3516
void sdm_spectrum_params_init(sdm_spectrum_params_t* p) { *p = sdm_spectrum_params_t{0.40f, 3, 1.0f, 2, 0.50f, 4, 0.9f}; }  // :3524-3530
bool sd_set_step_cache_ex(sdm_ctx_t* ctx, const sdm_cache_params_t* params, const sdm_cache_dit_params_t* cache_dit, const sdm_spectrum_params_t* spectrum) {
    if (cache_dit && std::isnan(cache_dit->residual_diff_threshold)) {
        set_error("sd_set_step_cache_ex: NaN parameter");
        return false;
    }
    if (spectrum && (std::isnan(spectrum->w) || std::isnan(spectrum->lam) || std::isnan(spectrum->flex_window) || std::isnan(spectrum->stop_percent))) {
        set_error("sd_set_step_cache_ex: NaN parameter");
        return false;
    }
    if (spectrum && (spectrum->m < 0 || spectrum->m > SpectrumState::MAX_K - 1)) {
        set_error("sd_set_step_cache_ex: spectrum m must be 0 .. 15 (the history holds max(m + 1, 6) <= 16 tensors)");
        return false;
    }
    if (!sd_set_step_cache(ctx, params)) return false;
    if (cache_dit) ctx->cache_dit_params = *cache_dit;
    if (spectrum) ctx->spectrum_params = *spectrum;
    return true;
}
bool sd_spectrum_schedule(const sdm_spectrum_params_t* params, int n_calls, uint8_t* predicted) {
    if (!params || n_calls < 0 || (n_calls > 0 && !predicted) || params->m < 0 || params->m > SpectrumState::MAX_K - 1) {
        set_error("sd_spectrum_schedule: bad arguments");
        return false;
    }
    SpectrumState s;
    s.init(SpectrumConfig{params->w, params->m, params->lam, params->window_size, params->flex_window, params->warmup_steps, params->stop_percent}, (size_t)n_calls);
    float weights[SpectrumState::MAX_K];
    int order[SpectrumState::MAX_K];
    for (int i = 0; i < n_calls; ++i) {
        predicted[i] = s.should_predict() ? 1 : 0;
        if (predicted[i])
            s.predict(weights, order);
        else
            s.update();
    }
    return true;
}
bool sd_spectrum_weights(const sdm_spectrum_params_t* params, const float* taus, int k, float tau_at, float* weights) {
    if (!params || !taus || !weights || k < 1 || k > SpectrumState::MAX_K || params->m < 0 || params->m > SpectrumState::MAX_K - 1) {
        set_error("sd_spectrum_weights: bad arguments");
        return false;
    }
    SpectrumState::weights(SpectrumConfig{params->w, params->m, params->lam, params->window_size, params->flex_window, params->warmup_steps, params->stop_percent}, taus, k, tau_at,
                           weights);
    return true;
}
bool sd_spectrum_kernels(sdm_ctx_t* ctx, const float* hist, int k, int64_t n, const float* weights, float w, float* out) {
    if (!hist || !weights || !out || k < 2 || k > SpectrumState::MAX_K || n < 1) {
        set_error("sd_spectrum_kernels: bad arguments");
        return false;
    }
    ggml_init_params ip{0, nullptr, true};
    ggml_context* c       = ggml_init(ip);
    const int64_t stride  = (n + 3) / 4 * 4;
    ggml_tensor* t_ring   = ggml_new_tensor_2d(c, GGML_TYPE_F32, stride, k);
    ggml_tensor* t_src    = ggml_new_tensor_1d(c, GGML_TYPE_F32, n);
    ggml_tensor* t_out    = ggml_new_tensor_1d(c, GGML_TYPE_F32, n);
    ggml_backend_buffer_t buf = ggml_backend_alloc_ctx_tensors(c, ctx->backend);
    if (!buf) {
        ggml_free(c);
        set_error("sd_spectrum_kernels: allocation failed");
        return false;
    }
    // the sampler's path: every tensor arrives in its ring slot through the push, rotated so that the ring wraps (slot of the j-th oldest = (j + 1) % k)
    StepCacheDevice dev(ctx->backend);
    bool ok = !dev.mode_exports_missing;
    int order[SpectrumState::MAX_K];
    for (int j = 0; ok && j < k; ++j) {
        order[j] = (j + 1) % k;
        ggml_backend_tensor_set(t_src, hist + (size_t)j * (size_t)n, 0, (size_t)n * sizeof(float));
        ok = dev.spectrum_push(t_src, t_ring, stride, order[j], n);
        ggml_backend_synchronize(ctx->backend);  // t_src is overwritten by the next upload
    }
    ok = ok && dev.spectrum_predict(t_ring, stride, k, order, k, weights, w, n, t_out);
    ggml_backend_synchronize(ctx->backend);
    if (ok)
        ggml_backend_tensor_get(t_out, out, 0, (size_t)n * sizeof(float));
    else
        set_error("sd_spectrum_kernels: the passes could not be run");
    ggml_backend_buffer_free(buf);
    ggml_free(c);
    return ok;
}
bool sd_step_cache_kernels_rel(sdm_ctx_t* ctx, const float* in, const float* prev_in, int64_t n, float c_in, float* sums) {
    if (!in || !prev_in || !sums || n < 1) {
        set_error("sd_step_cache_kernels_rel: bad arguments");
        return false;
    }
    ggml_init_params ip{0, nullptr, true};
    ggml_context* c    = ggml_init(ip);
    ggml_tensor* t_in  = ggml_new_tensor_1d(c, GGML_TYPE_F32, n);
    ggml_tensor* t_pin = ggml_new_tensor_1d(c, GGML_TYPE_F32, n);
    ggml_tensor* t_st  = ggml_new_tensor_1d(c, GGML_TYPE_F32, 4);
    ggml_backend_buffer_t buf = ggml_backend_alloc_ctx_tensors(c, ctx->backend);
    if (!buf) {
        ggml_free(c);
        set_error("sd_step_cache_kernels_rel: allocation failed");
        return false;
    }
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    ggml_backend_tensor_set(t_in, in, 0, (size_t)n * sizeof(float));
    ggml_backend_tensor_set(t_pin, prev_in, 0, (size_t)n * sizeof(float));
    ggml_backend_tensor_set(t_st, zero, 0, sizeof(zero));
    StepCacheDevice dev(ctx->backend);
    const bool ok = !dev.mode_exports_missing && dev.probe_rel(t_in, c_in, t_pin, n, t_st);
    if (ok) {
        float st4[4];
        ggml_backend_tensor_get(t_st, st4, 0, sizeof(st4));  // (synchronises the stream the pass was enqueued on)
        sums[0] = st4[0], sums[1] = st4[3];
    } else {
        ggml_backend_synchronize(ctx->backend);
        set_error("sd_step_cache_kernels_rel: the pass could not be run (size beyond the summation-depth bound?)");
    }
    ggml_backend_buffer_free(buf);
    ggml_free(c);
    return ok;
}
int sd_step_cache_trace(sdm_ctx_t* ctx, sdm_cache_step_t* out, int capacity) {
    const std::vector<sdm_cache_step_t>& t = ctx->step_cache.trace;
    for (int i = 0; out && i < capacity && i < (int)t.size(); ++i) out[i] = t[(size_t)i];
    return (int)t.size();
}
const char* sd_step_cache_status(sdm_ctx_t* ctx) { return ctx->step_cache.status.c_str(); }
float sd_t_to_sigma(sdm_ctx_t* ctx, float t) { return ctx->t_to_sigma(t); }
bool sd_step_cache_device_passes(sdm_ctx_t* ctx) { return StepCacheDevice(ctx->backend).on_device(); }
bool sd_step_cache_kernels(sdm_ctx_t* ctx, const float* in, const float* out, const float* prev_in, const float* prev_out, int64_t n, int k, int nb, float c_in, float* stats,
                           float* diff_out, float* prev_in_out, float* prev_out_out) {
    if (!in || !out || !prev_in || !stats || n < 1 || nb < 1 || k < 1 || k > 2) {
        set_error("sd_step_cache_kernels: bad arguments");
        return false;
    }
    ggml_init_params ip{0, nullptr, true};
    ggml_context* c = ggml_init(ip);
    ggml_tensor* t_in   = ggml_new_tensor_2d(c, GGML_TYPE_F32, n, nb);
    ggml_tensor* t_pin  = ggml_new_tensor_2d(c, GGML_TYPE_F32, n, nb);
    ggml_tensor* t_pout = ggml_new_tensor_2d(c, GGML_TYPE_F32, n, nb);
    ggml_tensor* t_out  = ggml_new_tensor_3d(c, GGML_TYPE_F32, n, k, nb);
    ggml_tensor* t_diff = ggml_new_tensor_3d(c, GGML_TYPE_F32, n, k, nb);
    ggml_tensor* t_st   = ggml_new_tensor_1d(c, GGML_TYPE_F32, 4);
    ggml_backend_buffer_t buf = ggml_backend_alloc_ctx_tensors(c, ctx->backend);
    if (!buf) {
        ggml_free(c);
        set_error("sd_step_cache_kernels: allocation failed");
        return false;
    }
    const size_t bytes = (size_t)n * nb * sizeof(float);
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    ggml_backend_tensor_set(t_in, in, 0, bytes);
    ggml_backend_tensor_set(t_out, out, 0, bytes * k);
    ggml_backend_tensor_set(t_pin, prev_in, 0, bytes);
    if (prev_out) ggml_backend_tensor_set(t_pout, prev_out, 0, bytes);
    ggml_backend_tensor_set(t_st, zero, 0, sizeof(zero));
    StepCacheDevice dev(ctx->backend);
    const bool ok = !dev.exports_missing && dev.probe(t_in, c_in, t_pin, n * nb, t_st) && dev.record(t_in, t_out, t_pin, t_pout, t_diff, n, k, nb, prev_out != nullptr, t_st);
    if (ok) {
        float st4[4];
        ggml_backend_tensor_get(t_st, st4, 0, sizeof(st4));  // (synchronises the stream the passes were enqueued on)
        memcpy(stats, st4, 3 * sizeof(float));
        if (diff_out) ggml_backend_tensor_get(t_diff, diff_out, 0, bytes * k);
        if (prev_in_out) ggml_backend_tensor_get(t_pin, prev_in_out, 0, bytes);
        if (prev_out_out) ggml_backend_tensor_get(t_pout, prev_out_out, 0, bytes);
    } else {
        ggml_backend_synchronize(ctx->backend);
        set_error("sd_step_cache_kernels: the passes could not be run (size beyond the summation-depth bound?)");
    }
    ggml_backend_buffer_free(buf);
    ggml_free(c);
    return ok;
}

// ---- latent previews (csrc/host/preview.hpp) -----------------------------------------------------------------------------------
bool sdm_set_preview_callback(sdm_ctx_t* ctx, sdm_preview_cb_t cb, int mode, int interval, bool denoised, bool noisy, void* data) {
    if (cb && (mode < SDM_PREVIEW_NONE || mode > SDM_PREVIEW_VAE)) {
        set_error("sdm_set_preview_callback: mode must be one of sdm_preview_t");
        return false;
    }
    PreviewState& pv = ctx->preview;
    pv.cb            = (cb && mode != SDM_PREVIEW_NONE) ? cb : nullptr;
    pv.user          = data;
    pv.mode          = pv.cb ? mode : SDM_PREVIEW_NONE;
    pv.interval      = interval;
    pv.denoised      = denoised;
    pv.noisy         = noisy;
    // off: every sampler path is the one without previews again.  What a preview allocated (preview.denoised, the capturing graphs' compute buffer, the upload tensor)
    // stays until the sampler state or the context goes: freeing a backend buffer makes the backend drop every cached plan, and a front end that installs a callback per
    // generation must not pay a re-plan of the step graph for it
    return true;
}
int sdm_preview_first_image(sdm_ctx_t* ctx) { return ctx->preview_current.first_image; }
int64_t sdm_preview_latent(sdm_ctx_t* ctx, float* out, int64_t capacity, float* in_scale) {
    const sdm_ctx_t::PreviewCurrent& cur = ctx->preview_current;
    if (!cur.active) return 0;
    if (in_scale) *in_scale = cur.in_scale;
    const int64_t n = std::min(cur.floats, capacity);
    if (out && n > 0) {
        if (cur.host)
            memcpy(out, cur.host, (size_t)n * sizeof(float));
        else
            ggml_backend_tensor_get(cur.dev, out, 0, (size_t)n * sizeof(float));
    }
    return cur.floats;
}
bool sdm_set_preview_projection(sdm_ctx_t* ctx, const float* proj, const float* bias, int c) {
    PreviewState& pv = ctx->preview;
    if (!proj) {
        pv.custom_proj.clear();
        pv.custom_c = 0;
        return true;
    }
    if (c < 1 || c > PREVIEW_MAX_CHANNELS) {
        set_error("sdm_set_preview_projection: 1 .. 128 channels");
        return false;
    }
    pv.custom_proj.assign(proj, proj + 3 * (size_t)c);
    for (int k = 0; k < 3; ++k) pv.custom_bias[k] = bias ? bias[k] : 0.0f;
    pv.custom_c = c;
    return true;
}
bool sdm_preview_device_passes(sdm_ctx_t* ctx) { return PreviewDevice(ctx->backend).on_device(); }
bool sdm_latent_preview(sdm_ctx_t* ctx, const float* latents, int w, int h, int c, int n, float in_scale, uint8_t* out_rgb) {
    const float *proj = nullptr, *bias = nullptr;
    if (!latents || !out_rgb || w < 1 || h < 1 || n < 1 || c < 1 || c > PREVIEW_MAX_CHANNELS || !preview_table(ctx, c, &proj, &bias)) {
        set_error("sdm_latent_preview: bad arguments (a NULL buffer, more than 128 channels, or no projection known for this channel count)");
        return false;
    }
    PreviewDevice pd(ctx->backend);
    if (pd.exports_missing) {
        set_error("sdm_latent_preview: the MI355X backend does not export its preview passes");
        return false;
    }
    if (!preview_proj_host_latent(ctx, pd, latents, w, h, c, n, in_scale, proj, bias, out_rgb)) {
        set_error("sdm_latent_preview: the pass could not be run");
        return false;
    }
    return true;
}
bool sdm_planar_to_u8(sdm_ctx_t* ctx, const float* chw, int w, int h, int n, uint8_t* out_rgb) {
    if (!chw || !out_rgb || w < 1 || h < 1 || n < 1) {
        set_error("sdm_planar_to_u8: bad arguments");
        return false;
    }
    PreviewDevice pd(ctx->backend);
    if (pd.exports_missing) {
        set_error("sdm_planar_to_u8: the MI355X backend does not export its preview passes");
        return false;
    }
    const int64_t plane = (int64_t)w * h;
    if (!pd.on_device()) return planar_to_u8_host(chw, plane, n, 1.0f, 0.0f, out_rgb);
    ggml_init_params ip{0, nullptr, true};
    ggml_context* c  = ggml_init(ip);
    ggml_tensor* t   = ggml_new_tensor_4d(c, GGML_TYPE_F32, w, h, 3, n);
    ggml_backend_buffer_t buf = ggml_backend_alloc_ctx_tensors(c, ctx->backend);
    if (!buf) {
        ggml_free(c);
        set_error("sdm_planar_to_u8: allocation failed");
        return false;
    }
    ggml_backend_tensor_set_async(ctx->backend, t, chw, 0, (size_t)plane * 3 * n * sizeof(float));
    const bool ok = pd.u8_k(ctx->backend, (const float*)t->data, plane, n, 1.0f, 0.0f, out_rgb);
    ggml_backend_synchronize(ctx->backend);
    if (!ok) set_error("sdm_planar_to_u8: the pass could not be enqueued");
    ggml_backend_buffer_free(buf);
    ggml_free(c);
    return ok;
}

bool sd_sample_latents(sdm_ctx_t* ctx, const sdm_img_gen_params_t* p, float* out_latents) {
    const int W = p->width / 8, H = p->height / 8, C = ctx->latent_channels();
    const size_t per = (size_t)W * H * C;
    const int group  = p->device_batch > 0 ? p->device_batch : p->batch_count;
    const double t0  = now_ms();
    ctx->stats.steps_skipped = 0;
    if (ctx->step_cache_would_arm(resolve_sample_method(ctx, p->sample_params.sample_method))) {
        const sdm_sample_params_t& sp = p->sample_params;
        // the reference re-enters its cache with the cond pointer a second time inside a skip-layer step; that is not restated: refused
        if (ctx->is_dit && !ctx->is_flux && sp.slg_scale != 0.0f && sp.slg_layers && sp.slg_layer_count > 0) {
            set_error("step cache: not available together with skip-layer guidance");
            return false;
        }
        if (ctx->pair_fn != nullptr && p->device_sampler) {
            set_error("step cache: not available with a CFG-pair exchange (the anchor condition lives on one rank only)");
            return false;
        }
    }
    if (ctx->variant != SDM_UNET_PLAIN) {  // inpaint / pix2pix UNets: the model input needs its extra channels
        const sdm_ctx_t::ConcatCondition& cs = ctx->concat_cond;
        if (!cs.set()) {
            set_error("model needs c_concat: no concat condition is set (sd_set_concat_condition)");
            return false;
        }
        if (cs.w != W || cs.h != H || (cs.n != 1 && cs.n != p->batch_count)) {
            set_error("concat condition is [" + std::to_string(cs.w) + "," + std::to_string(cs.h) + "," + std::to_string(cs.cc) + "," + std::to_string(cs.n) + "], the request needs [" +
                      std::to_string(W) + "," + std::to_string(H) + "," + std::to_string(cs.cc) + ", 1 or " + std::to_string(p->batch_count) + "]");
            return false;
        }
        const GuidancePlan gp = resolve_guidance_plan(ctx, p);
        if (gp.img_cfg != 1.0f && !p->uncond.c_crossattn) {
            set_error("image guidance (img_cfg != 1) needs the uncond conditioning: its text is the third condition's text");
            return false;
        }
        if (gp.use_img_uncond) {  // the third branch
            const sdm_sample_params_t& sp = p->sample_params;
            if (ApgParams{sp.apg_eta, sp.apg_momentum, sp.apg_norm_threshold, sp.apg_norm_threshold_smoothing}.enabled()) {
                set_error("image guidance: a third branch is not available together with adaptive projected guidance");
                return false;
            }
            if (ctx->step_cache_would_arm(resolve_sample_method(ctx, sp.sample_method))) {
                set_error("image guidance: a third branch is not available together with a step cache");
                return false;
            }
            if (ctx->pair_fn != nullptr) {
                set_error("image guidance: a third branch is not available with a CFG-pair exchange");
                return false;
            }
        }
    }
    if (ctx->preview.on() && ctx->pair_fn != nullptr && p->device_sampler) {
        set_error("preview: not available with a CFG-pair exchange on the device-resident sampler (both ranks would synchronise and deliver the same frames)");
        return false;
    }
    for (int b0 = 0; b0 < p->batch_count; b0 += group) {
        const int nb = std::min(group, p->batch_count - b0);
        if (p->device_sampler) {
            bool handled = false;
            if (!sample_group_device(ctx, p, b0, nb, out_latents + b0 * per, &handled)) return false;
            if (handled) {
                ctx->stats.steps_skipped += ctx->step_cache.total_steps_skipped();
                continue;
            }  // otherwise (cond / uncond shapes differ): the host loop below
        }
        if (!sample_group(ctx, p, b0, nb, out_latents + b0 * per)) return false;
        ctx->stats.steps_skipped += ctx->step_cache.total_steps_skipped();
    }
    ctx->stats.last_sample_ms = now_ms() - t0;
    return true;
}

static inline uint8_t float_to_u8(float v) {  // preprocessing.hpp:27-35
    if (v <= 0.0f) return 0;
    if (v >= 1.0f) return 255;
    return (uint8_t)(v * 255.0f + 0.5f);
}

// planar CHW floats in [0, 1] -> interleaved RGB bytes (preprocessing_tensor_frame_to_sd_image, src/runtime/preprocessing.hpp:37-60)
static void planar_rgb_to_u8(const float* f, size_t pix, uint8_t* d) {
    parallel_chunks(pix, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; ++i) {
            d[i * 3 + 0] = float_to_u8(f[i]);
            d[i * 3 + 1] = float_to_u8(f[pix + i]);
            d[i * 3 + 2] = float_to_u8(f[2 * pix + i]);
        }
    });
}
// the same conversion on caller memory — tests only (bit-exact against the reference's preprocessing.hpp compiled into oracle/_ref)
void sd_planar_rgb_to_u8(const float* chw, int width, int height, uint8_t* out) { planar_rgb_to_u8(chw, (size_t)width * height, out); }

bool sdm_generate_image(sdm_ctx_t* ctx, const sdm_img_gen_params_t* p, sdm_image_t** images_out, int* num_images_out) {
    const int W = p->width / 8, H = p->height / 8, C = ctx->latent_channels();
    const size_t per = (size_t)W * H * C;
    std::vector<float> latents(per * p->batch_count);
    if (!sd_sample_latents(ctx, p, latents.data())) return false;
    const int PW = W * 8, PH = H * 8;
    const size_t pix = (size_t)PW * PH;
    sdm_image_t* imgs = (sdm_image_t*)calloc(p->batch_count, sizeof(sdm_image_t));  // stable-diffusion.cpp:5398-5410
    std::vector<float> rgb(pix * 3 * p->batch_count);
    const int group = p->device_batch > 0 ? p->device_batch : p->batch_count;
    double dec_ms   = 0;
    for (int b0 = 0; b0 < p->batch_count; b0 += group) {
        const int nb = std::min(group, p->batch_count - b0);
        if (!(ctx->tae_for_images ? sd_tae_decode : sd_vae_decode)(ctx, latents.data() + b0 * per, W, H, C, nb, rgb.data() + (size_t)b0 * pix * 3)) {
            sdm_free_images(imgs, p->batch_count);
            return false;
        }
        dec_ms += ctx->stats.last_decode_ms;
    }
    ctx->stats.last_decode_ms = dec_ms;
    for (int b = 0; b < p->batch_count; ++b) {
        imgs[b].width   = PW;
        imgs[b].height  = PH;
        imgs[b].channel = 3;
        imgs[b].data    = (uint8_t*)malloc(pix * 3);
        const float* f  = rgb.data() + (size_t)b * pix * 3;
        uint8_t* d      = imgs[b].data;
        planar_rgb_to_u8(f, pix, d);
    }
    *images_out     = imgs;
    *num_images_out = p->batch_count;
    return true;
}

void sdm_free_images(sdm_image_t* images, int num_images) {
    if (!images) return;
    for (int i = 0; i < num_images; ++i) free(images[i].data);
    free(images);
}

void sd_philox_randn(uint64_t seed, uint32_t offset, uint32_t n, float* out) {
    PhiloxRNG r(seed);
    r.offset = offset;
    std::vector<float> v = r.randn(n);
    memcpy(out, v.data(), n * sizeof(float));
}
void sd_philox_uint32(uint64_t seed, uint32_t offset, uint32_t n, uint32_t* out) {
    for (uint32_t i = 0; i < n; ++i) PhiloxRNG::words(seed, offset, i, out + 4 * (size_t)i);
}
int sd_get_sigmas(int steps, float* out) {
    static CompVisDenoiser d;
    std::vector<float> s = d.get_sigmas(steps);
    memcpy(out, s.data(), s.size() * sizeof(float));
    return (int)s.size();
}
void sd_set_guidance(sdm_ctx_t* ctx, float guidance) { ctx->guidance = guidance; }
// the host sampler's CFG combine on n floats (cfg_guided, sampler.hpp) — exported so that tests can hold it bit-for-bit against the reference's own
// ClassifierFreeGuidance::forward compiled into oracle/_ref (src/runtime/guidance.cpp:149-179)
// The host sampler's loop — sigma ladder, initial noise, per-step scalings / timestep, ancestral step, update, Philox noise order — on ONE image of n floats
// with a SYNTHETIC model in place of the network: denoised = x * (1 / (1 + sigma)) + 0.01 * sigma  (plain f32 arithmetic the reference-side wrapper
// oracle/ref_denoiser_wrap.cpp states identically).  family: 0 = CompVis (SD1.x / SDXL), 1 = discrete flow (SD3.x, shift 3), 2 = FLUX flow; method: the
// sdm_sample_method_t value; eta: INFINITY = the method's default.  aux (optional, 5 floats per step): c_skip, c_out, c_in, t, sigma — what the loop fed the model.
// Tests only (tests/test_host_logic.py: bit-for-bit against the reference's src/runtime/denoiser.hpp compiled into oracle/_ref).
int sd_sample_synthetic(int family, int steps, int image_seq_len, int64_t n, uint64_t seed, int method, float eta, float* out, float* aux) {
    if (steps < 1 || n < 1 || family < 0 || family > 2) return -1;
    CompVisDenoiser cv;
    DiscreteFlowDenoiser fl;
    FluxFlowDenoiser fx;
    const bool flow = family != 0;
    if (eta == INFINITY) eta = method == SDM_EULER_A_SAMPLE_METHOD ? 1.0f : 0.0f;
    const std::vector<float> sigmas = family == 0 ? cv.get_sigmas((uint32_t)steps) : (family == 1 ? fl.get_sigmas((uint32_t)steps) : fx.get_sigmas((uint32_t)steps, image_seq_len));
    PhiloxRNG rng(seed);
    std::vector<float> x = rng.randn((uint32_t)n), den((size_t)n), nz;
    for (int64_t k = 0; k < n; ++k) x[k] = 0.0f + x[k] * sigmas[0];
    for (int i = 0; i + 1 < (int)sigmas.size(); ++i) {
        const float sigma = sigmas[i], sigma_to = sigmas[i + 1];
        float c_skip, c_out, c_in;
        if (family == 0) cv.scalings(sigma, c_skip, c_out, c_in);
        else if (family == 1) fl.scalings(sigma, c_skip, c_out, c_in);
        else fx.scalings(sigma, c_skip, c_out, c_in);
        const float t = family == 0 ? cv.sigma_to_t(sigma) : (family == 1 ? fl.sigma_to_t(sigma) : sigma);
        if (aux) {
            float* a = aux + 5 * i;
            a[0] = c_skip, a[1] = c_out, a[2] = c_in, a[3] = t, a[4] = sigma;
        }
        const float g = 1.0f / (1.0f + sigma), h = 0.01f * sigma;
        for (int64_t k = 0; k < n; ++k) den[k] = x[k] * g + h;
        float sigma_down = 0.f, sigma_up = 0.f, alpha_scale = 1.f;
        if (method == SDM_EULER_A_SAMPLE_METHOD && sigma_to != 0.f && eta != 0.f) {
            if (flow) ancestral_step_flow(sigma, sigma_to, eta, sigma_down, sigma_up, alpha_scale);
            else ancestral_step(sigma, sigma_to, eta, sigma_down, sigma_up);
        }
        sampler_update(x.data(), den.data(), (size_t)n, 1, method == SDM_EULER_A_SAMPLE_METHOD, flow, sigma, sigma_to, eta, sigma_down, sigma_up, alpha_scale,
                       [&](int) -> const float* {
                           nz = rng.randn((uint32_t)n);
                           return nz.data();
                       });
    }
    memcpy(out, x.data(), sizeof(float) * (size_t)n);
    return (int)sigmas.size();
}
// sd_sample_synthetic with a scheduler and every implemented method (the loop sample_group runs, on the synthetic model); aux: 5 floats per model call, in call order
int sd_sample_synthetic2(int family, int steps, int image_seq_len, int64_t n, uint64_t seed, int method, int scheduler, float eta, float* out, float* aux, int aux_calls) {
    if (steps < 1 || n < 1 || family < 0 || family > 4 || !sample_method_supported(method)) return -1;  // family 4: CompVis with the v-prediction scalings
    CompVisDenoiser cv;
    DiscreteFlowDenoiser fl;
    FluxFlowDenoiser fx;
    const int fam   = (family == 3 || family == 4) ? 0 : family;
    const bool flow = fam != 0;
    if (scheduler == SDM_SCHEDULER_COUNT) scheduler = (method == SM_LCM || method == SM_TCD) ? SCHED_LCM : (method == SM_DDIM_TRAILING ? SCHED_SIMPLE : (fam == 2 ? SCHED_FLUX : SCHED_DISCRETE));
    if (!scheduler_supported(scheduler)) return -1;
    if (eta == INFINITY) eta = default_eta(method);
    if (method == SM_DDIM_TRAILING) method = SM_EULER_A;
    std::vector<float> sigmas((size_t)steps + 2);
    const int ns = sd_get_sigmas_sched(family, scheduler, steps, image_seq_len, 0.f, sigmas.data());
    if (ns < 2) return -1;
    sigmas.resize((size_t)ns);
    PhiloxRNG rng(seed);
    std::vector<float> x = rng.randn((uint32_t)n);
    for (int64_t k = 0; k < n; ++k) x[k] = 0.0f + x[k] * sigmas[0];
    int calls  = 0;
    auto model = [&](const float* xin, float sigma, float* den, float* unc, int /*step*/) {
        float c_skip, c_out, c_in;
        if (family == 4) {  // CompVisVDenoiser::get_scalings, sigma_data = 1 (the expressions sdm_ctx_t::scalings uses for SDM_V_PRED)
            const float sigma_data = 1.0f;
            c_skip = sigma_data * sigma_data / (sigma * sigma + sigma_data * sigma_data);
            c_out  = -sigma * sigma_data / std::sqrt(sigma * sigma + sigma_data * sigma_data);
            c_in   = 1.0f / std::sqrt(sigma * sigma + sigma_data * sigma_data);
        } else if (fam == 0) cv.scalings(sigma, c_skip, c_out, c_in);
        else if (fam == 1) fl.scalings(sigma, c_skip, c_out, c_in);
        else fx.scalings(sigma, c_skip, c_out, c_in);
        const float t = fam == 0 ? cv.sigma_to_t(sigma) : (fam == 1 ? fl.sigma_to_t(sigma) : sigma);
        if (aux && calls < aux_calls) {
            float* a = aux + 5 * (size_t)calls;
            a[0] = c_skip, a[1] = c_out, a[2] = c_in, a[3] = t, a[4] = sigma;
        }
        ++calls;
        const float g = 1.0f / (1.0f + sigma), h = 0.01f * sigma;
        for (int64_t k = 0; k < n; ++k) den[k] = xin[k] * g + h;
        if (unc) {  // the synthetic model's unconditional prediction (the CFG++ methods)
            const float gu = 0.9f / (1.0f + sigma), hu = -0.02f * sigma;
            for (int64_t k = 0; k < n; ++k) unc[k] = xin[k] * gu + hu;
        }
        return true;
    };
    if (method == SM_EULER || method == SM_EULER_A) {
        std::vector<float> den((size_t)n), nz;
        for (int i = 0; i + 1 < (int)sigmas.size(); ++i) {
            const float sigma = sigmas[i], sigma_to = sigmas[i + 1];
            model(x.data(), sigma, den.data(), nullptr, i + 1);
            float sigma_down = 0.f, sigma_up = 0.f, alpha_scale = 1.f;
            if (method == SM_EULER_A && sigma_to != 0.f && eta != 0.f) {
                if (flow) ancestral_step_flow(sigma, sigma_to, eta, sigma_down, sigma_up, alpha_scale);
                else ancestral_step(sigma, sigma_to, eta, sigma_down, sigma_up);
            }
            sampler_update(x.data(), den.data(), (size_t)n, 1, method == SM_EULER_A, flow, sigma, sigma_to, eta, sigma_down, sigma_up, alpha_scale, [&](int) -> const float* {
                nz = rng.randn((uint32_t)n);
                return nz.data();
            });
        }
    } else if (!run_sampler_generic(method, model, x, sigmas, [&](float* dst) {
                   const std::vector<float> nz = rng.randn((uint32_t)n);
                   memcpy(dst, nz.data(), sizeof(float) * (size_t)n);
               }, eta, flow, 1, [&](int, uint32_t cnt, float* dst) {
                   const std::vector<float> nz = rng.randn(cnt);
                   memcpy(dst, nz.data(), sizeof(float) * cnt);
               })) {
        return -1;
    }
    memcpy(out, x.data(), sizeof(float) * (size_t)n);
    return calls;
}
int sd_get_sigmas_sched(int family, int scheduler, int steps, int image_seq_len, float shift, float* out) {
    if (family < 0 || family > 4 || steps < 0 || !scheduler_supported(scheduler)) return -1;
    std::vector<float> s;
    if (scheduler == SCHED_FLUX) {
        FluxFlowDenoiser d;
        s = d.get_sigmas((uint32_t)steps, image_seq_len);
    } else if (family == 0 || family == 3 || family == 4) {
        static const CompVisDenoiser d;
        s = scheduler_sigmas(scheduler, (uint32_t)steps, d.sigma_min(), d.sigma_max(), [&](float t) { return d.t_to_sigma(t); }, family == 3 ? 1 : 0);
    } else if (family == 1) {
        DiscreteFlowDenoiser d;
        if (shift > 0.f) d.shift = shift;
        s = scheduler_sigmas(scheduler, (uint32_t)steps, d.sigma_min(), d.sigma_max(), [&](float t) { return d.t_to_sigma(t); }, -1);
    } else {
        FluxFlowDenoiser d;
        if (shift > 0.f) d.shift = shift;
        s = scheduler_sigmas(scheduler, (uint32_t)steps, d.sigma_min(), d.sigma_max(), [&](float t) { return d.t_to_sigma(t); }, -1);
    }
    memcpy(out, s.data(), s.size() * sizeof(float));
    return (int)s.size();
}
// adaptive projected guidance over `steps` successive denoise calls of one image (momentum carried), for the bit-exact test against the reference's guidance.cpp
void sd_apg_sequence(const float* cond, const float* uncond, int64_t n, int steps, float scale, float eta, float momentum, float norm_threshold, float norm_threshold_smoothing, float* out) {
    const ApgParams prm{eta, momentum, norm_threshold, norm_threshold_smoothing};
    std::vector<float> buf;
    for (int s = 0; s < steps; ++s) apg_guided(cond + (size_t)s * n, uncond + (size_t)s * n, (size_t)n, scale, prm, buf, out + (size_t)s * n);
}
void sd_cfg_combine(const float* cond, const float* uncond, int64_t n, float scale, float* out) {
    for (int64_t k = 0; k < n; ++k) out[k] = cfg_guided(cond[k], uncond[k], scale);
}
// ---- inpaint / pix2pix UNets: image guidance, the concat condition and how it is made from pixels ----------------------------------------------
// ClassifierFreeGuidance::forward's three forms (guidance.cpp:162-176) by which predictions exist: uncond or img_uncond may be NULL
void sd_cfg_combine3(const float* cond, const float* uncond, const float* img_uncond, int64_t n, float txt_cfg, float img_cfg, float* out) {
    for (int64_t k = 0; k < n; ++k)
        out[k] = (uncond && img_uncond) ? cfg_guided3(cond[k], uncond[k], img_uncond[k], txt_cfg, img_cfg)
                 : uncond               ? cfg_guided(cond[k], uncond[k], txt_cfg)
                 : img_uncond           ? cfg_guided(cond[k], img_uncond[k], txt_cfg)
                                        : cond[k];
}
bool sd_set_img_cfg(sdm_ctx_t* ctx, float img_cfg) {
    if (std::isnan(img_cfg)) {
        set_error("sd_set_img_cfg: NaN");
        return false;
    }
    ctx->img_cfg = img_cfg;
    ctx->guidance_status.clear();
    if (ctx->variant == SDM_UNET_PLAIN && std::isfinite(img_cfg) && img_cfg != 1.0f) {
        // resolve_guidance's warning (stable-diffusion.cpp:4242-4247): accepted and ignored
        ctx->guidance_status = "3-conditioning CFG is not supported with this model, disabling it for better performance";
        set_error(ctx->guidance_status);
    }
    return true;
}
bool sd_set_concat_condition(sdm_ctx_t* ctx, const float* concat, const float* img_uncond_concat, int w, int h, int cc, int n) {
    sdm_ctx_t::ConcatCondition& s = ctx->concat_cond;
    if (!concat) {
        s = sdm_ctx_t::ConcatCondition();
        return true;
    }
    if (ctx->variant == SDM_UNET_PLAIN) {
        set_error("sd_set_concat_condition: the model takes no c_concat (a plain context)");
        return false;
    }
    if (cc != ctx->concat_channels() || w < 1 || h < 1 || n < 1) {
        set_error("sd_set_concat_condition: the model takes a [w,h," + std::to_string(ctx->concat_channels()) + ",n] concat, got cc = " + std::to_string(cc));
        return false;
    }
    const size_t plane = (size_t)w * h, one = plane * cc, total = one * n;
    s.concat.assign(concat, concat + total);
    if (img_uncond_concat) {
        s.img_uncond.assign(img_uncond_concat, img_uncond_concat + total);
    } else {
        // the reference's default (stable-diffusion.cpp:5145, 5168, 5173): inpaint keeps the mask channel and zeroes the masked latent, pix2pix is all zeros
        s.img_uncond.assign(total, 0.0f);
        if (ctx->variant == SDM_UNET_INPAINT)
            for (int b = 0; b < n; ++b) memcpy(&s.img_uncond[(size_t)b * one], concat + (size_t)b * one, plane * sizeof(float));
    }
    s.w = w, s.h = h, s.cc = cc, s.n = n;
    return true;
}
// sd::ops::round (tensor.hpp:1089-1092: std::round, halves away from zero — 0.5 becomes 1) followed by interpolate(..., NearestMax) to w/8 x h/8 (:1346-1360: the max over
// the source block [o * in / out, ceil((o + 1) * in / out)) per axis): stable-diffusion.cpp:4986-5010
bool sd_latent_mask(const float* mask, int w, int h, float* out) {
    if (!mask || !out || w < 8 || h < 8 || w % 8 || h % 8) {
        set_error("sd_latent_mask: width and height must be positive multiples of 8");
        return false;
    }
    const int64_t lw = w / 8, lh = h / 8;
    for (int64_t oy = 0; oy < lh; ++oy)
        for (int64_t ox = 0; ox < lw; ++ox) {
            const int64_t x0 = ox * w / lw, x1 = std::min<int64_t>(w, ((ox + 1) * w + lw - 1) / lw), y0 = oy * h / lh, y1 = std::min<int64_t>(h, ((oy + 1) * h + lh - 1) / lh);
            float v = std::numeric_limits<float>::lowest();
            for (int64_t y = y0; y < y1; ++y)
                for (int64_t x = x0; x < x1; ++x) v = std::max(v, static_cast<float>(std::round(static_cast<double>(mask[y * w + x]))));
            out[oy * lw + ox] = v;
        }
    return true;
}
// sd::ops::max_pool_2d(latent_mask, {3, 3}, {1, 1}, {1, 1}) (tensor.hpp:1473-1544; stable-diffusion.cpp:5197-5203): cells outside the map do not take part
bool sd_mask_max_pool3(const float* in, int w, int h, float* out) {
    if (!in || !out || w < 1 || h < 1 || in == out) {
        set_error("sd_mask_max_pool3: bad arguments");
        return false;
    }
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            float v = std::numeric_limits<float>::lowest();
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int yy = y + dy, xx = x + dx;
                    if (yy >= 0 && yy < h && xx >= 0 && xx < w) v = std::max(v, in[(size_t)yy * w + xx]);
                }
            out[(size_t)y * w + x] = v;
        }
    return true;
}
// prepare_image_generation_latents for the UNet inpaint and edit models (stable-diffusion.cpp:4986-5010, 5127-5173, 5197-5203).  Both encodes draw from Philox(seed)
// at offset 0 (sd_vae_encode's convention; the reference continues one stream from the init image to the masked image)
bool sd_make_inpaint_condition(sdm_ctx_t* ctx, const float* rgb, const float* mask, int w, int h, uint64_t seed, float* concat_out, float* img_uncond_concat_out,
                               float* denoise_mask_out, float* init_latent_out) {
    if (ctx->variant == SDM_UNET_PLAIN) {
        set_error("sd_make_inpaint_condition: the model takes no c_concat (a plain context)");
        return false;
    }
    if (!rgb || !concat_out || w < 8 || h < 8 || w % 8 || h % 8 || (ctx->variant == SDM_UNET_INPAINT && !mask)) {
        set_error("sd_make_inpaint_condition: bad arguments (an image, sizes that are multiples of 8, and on an inpaint model a mask)");
        return false;
    }
    const int lw = w / 8, lh = h / 8, zc = ctx->latent_channels();
    const size_t plane = (size_t)lw * lh, pix = (size_t)w * h;
    if (ctx->variant == SDM_UNET_PIX2PIX) {  // the encoded image; the third condition sees zeros; no denoise mask
        if (!sd_vae_encode(ctx, rgb, w, h, 1, seed, concat_out, nullptr)) return false;
        if (img_uncond_concat_out) std::fill(img_uncond_concat_out, img_uncond_concat_out + plane * zc, 0.0f);
        if (init_latent_out) memcpy(init_latent_out, concat_out, plane * zc * sizeof(float));
        return true;
    }
    std::vector<float> m(pix), masked(pix * 3);
    for (size_t i = 0; i < pix; ++i) m[i] = static_cast<float>(std::round(static_cast<double>(mask[i])));
    for (int c = 0; c < 3; ++c)
        for (size_t i = 0; i < pix; ++i) masked[c * pix + i] = ((1.0f - m[i]) * (rgb[c * pix + i] - 0.5f)) + 0.5f;  // stable-diffusion.cpp:5132
    if (!sd_latent_mask(mask, w, h, concat_out)) return false;                                                   // concat = latent mask | masked-image latent
    if (!sd_vae_encode(ctx, masked.data(), w, h, 1, seed, concat_out + plane, nullptr)) return false;
    if (img_uncond_concat_out) {
        memcpy(img_uncond_concat_out, concat_out, plane * sizeof(float));
        std::fill(img_uncond_concat_out + plane, img_uncond_concat_out + plane * (1 + zc), 0.0f);
    }
    if (denoise_mask_out && !sd_mask_max_pool3(concat_out, lw, lh, denoise_mask_out)) return false;
    if (init_latent_out && !sd_vae_encode(ctx, rgb, w, h, 1, seed, init_latent_out, nullptr)) return false;
    return true;
}
// the device-resident sampler's two glue stages on caller memory: the node chains sample_group_device emits (the model-input chain as it stands in front of
// UNetModel::forward's concat, the three-term combine as in the step graph's tail), computed as graphs on the context's backend — one launch each on the MI355X
// backend (plan_model_input / plan_guidance3), the plain nodes on any other
bool sd_guidance_kernels(sdm_ctx_t* ctx, const float* x, float c_in, const float* concat, int w, int h, int c, int cc, int k, int nb, bool concat_per_image, float* xin_out,
                         const float* e3, float txt_cfg, float img_cfg, float* guided_out) {
    if (w < 1 || h < 1 || c < 1 || nb < 1 || (xin_out && (!x || !concat || cc < 1 || k < 1)) || (guided_out && !e3)) {
        set_error("sd_guidance_kernels: bad arguments");
        return false;
    }
    const int64_t per = (int64_t)w * h * c;
    const float sc[9] = {c_in, txt_cfg, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, img_cfg};  // the step graph's scalar tensor: [0] c_in, [1] txt_cfg, [8] img_cfg
    if (xin_out) {
        Runner r;
        r.backend    = ctx->backend;
        r.graph_size = 256;
        const int rows = concat_per_image ? k * nb : k;
        auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
            ggml_context* gc = g.ctx;
            ggml_tensor* tsc = ggml_new_tensor_1d(gc, GGML_TYPE_F32, 9);
            ggml_set_input(tsc);
            in.push_back({tsc, sc, sizeof(sc)});
            ggml_tensor* tx = ggml_new_tensor_4d(gc, GGML_TYPE_F32, w, h, c, nb);
            ggml_set_input(tx);
            in.push_back({tx, x, ggml_nbytes(tx)});
            ggml_tensor* tcat = ggml_new_tensor_4d(gc, GGML_TYPE_F32, w, h, cc, rows);
            ggml_set_input(tcat);
            in.push_back({tcat, concat, ggml_nbytes(tcat)});
            ggml_tensor* xin = ggml_mul(gc, tx, ggml_view_1d(gc, tsc, 1, 0));
            if (k > 1) {
                ggml_tensor* flat = ggml_reshape_3d(gc, xin, per, 1, nb);
                ggml_tensor* rep  = ggml_repeat(gc, flat, ggml_new_tensor_3d(gc, GGML_TYPE_F32, per, k, nb));
                xin               = ggml_reshape_4d(gc, rep, w, h, c, (int64_t)k * nb);
            }
            ggml_tensor* cat = tcat;
            if (cat->ne[3] != xin->ne[3]) cat = ggml_repeat(gc, cat, ggml_new_tensor_4d(gc, GGML_TYPE_F32, w, h, cc, xin->ne[3]));
            return ggml_concat(gc, xin, cat, 2);
        };
        if (!r.compute(build, xin_out, (size_t)w * h * (c + cc) * k * nb * sizeof(float))) return false;
    }
    if (guided_out) {
        Runner r;
        r.backend    = ctx->backend;
        r.graph_size = 256;
        auto build = [&](GraphCtx& g, std::vector<HostInput>& in) {
            ggml_context* gc = g.ctx;
            ggml_tensor* tsc = ggml_new_tensor_1d(gc, GGML_TYPE_F32, 9);
            ggml_set_input(tsc);
            in.push_back({tsc, sc, sizeof(sc)});
            ggml_tensor* t3 = ggml_new_tensor_3d(gc, GGML_TYPE_F32, per, 3, nb);
            ggml_set_input(t3);
            in.push_back({t3, e3, ggml_nbytes(t3)});
            auto S = [&](int j) { return ggml_view_1d(gc, tsc, 1, (size_t)j * sizeof(float)); };
            ggml_tensor* ec = ggml_view_3d(gc, t3, per, 1, nb, t3->nb[1], t3->nb[2], 0);
            ggml_tensor* eu = ggml_view_3d(gc, t3, per, 1, nb, t3->nb[1], t3->nb[2], t3->nb[1]);
            ggml_tensor* ei = ggml_view_3d(gc, t3, per, 1, nb, t3->nb[1], t3->nb[2], 2 * t3->nb[1]);
            ggml_tensor* a1 = ggml_add(gc, ei, ggml_mul(gc, ggml_sub(gc, eu, ei), S(8)));
            ggml_tensor* s2 = ggml_mul(gc, ggml_sub(gc, ec, eu), S(1));
            return ggml_add(gc, a1, s2);
        };
        if (!r.compute(build, guided_out, (size_t)per * nb * sizeof(float))) return false;
    }
    return true;
}
int sd_probe_unet_variant(const char* path) {
    ModelFile mf;
    if (!path || !read_model_file(path, mf)) {
        set_error(path ? mf.error : std::string("sd_probe_unet_variant: NULL path"));
        return -1;
    }
    const NameDialect dialect;  // (the first conv's name does not depend on the family's block layout)
    const std::string want = "model.diffusion_model.input_blocks.0.0.weight";
    for (const FileTensor& t : mf.tensors)
        for (const char* prefix : {"", "unet."}) {  // diffusers keeps one file per sub-model whose names carry no component prefix
            if (canonical_tensor_name(std::string(prefix) + t.name, dialect) != want) continue;
            const int64_t ic = t.n_dims >= 3 ? t.ne[2] : 0;
            if (ic == 4) return SDM_UNET_PLAIN;
            if (ic == 9) return SDM_UNET_INPAINT;
            if (ic == 8) return SDM_UNET_PIX2PIX;
            set_error("sd_probe_unet_variant: input_blocks.0.0.weight has " + std::to_string(ic) + " input channels (4, 9 or 8 expected)");
            return -1;
        }
    set_error("sd_probe_unet_variant: the file holds no model.diffusion_model.input_blocks.0.0.weight");
    return -1;
}
bool sd_set_vae_conv2d_scale(sdm_ctx_t* ctx, float scale) {
    if (!ctx || !(scale > 0.f) || !std::isfinite(scale)) {
        set_error("sd_set_vae_conv2d_scale: the scale must be a finite positive number");
        return false;
    }
    ctx->vae_conv2d_scale = scale;
    ctx->vae.set_conv2d_scale(scale);
    if (ctx->vae_enc_ready) ctx->vae_enc.set_conv2d_scale(scale);
    return true;
}
void sd_set_pair_exchange(sdm_ctx_t* ctx, sd_pair_exchange_fn fn, void* user, int branch) {
    ctx->pair_fn     = fn;
    ctx->pair_user   = user;
    ctx->pair_branch = branch != 0;
}
int sd_get_flux_sigmas(int steps, int image_seq_len, float* out) {
    FluxFlowDenoiser d;
    std::vector<float> s = d.get_sigmas(steps, image_seq_len);
    memcpy(out, s.data(), s.size() * sizeof(float));
    return (int)s.size();
}
int sd_gen_flux_pe(int h, int w, int patch_size, int context_len, const int* axes_dim, int n_axes, float theta, float* out) {
    std::vector<float> pe = gen_flux_pe(h, w, patch_size, context_len, std::vector<int>(axes_dim, axes_dim + n_axes), theta);
    memcpy(out, pe.data(), pe.size() * sizeof(float));
    return (int)pe.size();
}
int sd_get_flow_sigmas(int steps, float shift, float* out) {
    DiscreteFlowDenoiser d;
    d.shift              = shift;
    std::vector<float> s = d.get_sigmas(steps);
    memcpy(out, s.data(), s.size() * sizeof(float));
    return (int)s.size();
}
float sd_sigma_to_t(float sigma) {
    static CompVisDenoiser d;
    return d.sigma_to_t(sigma);
}
void sd_get_stats(sdm_ctx_t* ctx, sd_stats_t* out) {
    ctx->stats.host_build_ms  = ctx->unet_runner.build_ms;
    ctx->stats.host_alloc_ms  = ctx->unet_runner.alloc_ms;
    ctx->stats.host_submit_ms = ctx->unet_runner.submit_ms;
    ctx->stats.graph_cache_hits = ctx->unet_runner.cache_hits;
    *out                      = ctx->stats;
}

}  // extern "C"
