// step_cache.hpp — the reference's step caches, restated on the host: the condition-level caches EasyCache (DiT families; src/runtime/easycache.hpp), UCache (UNet
// families; src/runtime/ucache.hpp) and CacheDIT (DiT families; CacheDitConditionState, src/runtime/cache_dit.hpp:638-894 — what `dbcache`, `taylorseer` and
// `cache-dit` all run through), their set-up (src/runtime/sample-cache.cpp:5-146, 176-212) and the per-step dispatcher (sample-cache.cpp:214-291) the denoise call
// wraps around every model forward (src/stable-diffusion.cpp:2688, 2779-2795, 2817); and Spectrum (src/runtime/spectrum.hpp), which sits beside that dispatcher and
// replaces whole denoise calls (stable-diffusion.cpp:2583-2590, 2667-2679, 2885-2887).
//
// Both caches keep, per condition, diff = output - input of the last COMPUTED step (src/runtime/condition_cache_utils.hpp:10-36) and, for the anchor condition, the
// previous input and output.  In front of the anchor's forward they measure mean |input - prev_input|, scale it by the last observed output-change / input-change
// ratio and add it to an accumulator; while the accumulator stays under the threshold the step's outputs are rebuilt as input + diff (:38-60) and no model runs.
//
// The ARRAYS (prev_input, prev_output, the diffs) live with the loop that owns the data — host vectors in the host loop (HostStepCacheStore below), device tensors
// in the device-resident sampler — so the states here keep the reference's fields except those containers, whose presence is tracked by flags, and the two hooks are
// split where the reference touches data: before_condition() says what the caller has to do (compute / apply the diff / measure the input change and ask
// decide()), after_condition() takes the two means the reference accumulates in its own loops.  Order of operations as in the reference, line for line.
//
// CacheDIT keeps the same arrays and hooks; its decision is the relative L1 change of the anchor's input, sum |prev_in - in| / (sum |prev_in| + 1e-6), against a fixed
// threshold.  The block-level CacheDitState of the same file is used nowhere by the reference's sampler and is not restated.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "sampler.hpp"
#include "sd-mi355x.h"

namespace sdmi {

enum StepCacheAction { SC_COMPUTE = 0, SC_APPLY = 1, SC_MEASURE = 2 };

// what EasyCacheState and UCacheState share field for field (easycache.hpp:25-48, ucache.hpp:32-56) and the methods that read alike in both
struct ConditionCacheState {
    float start_sigma     = std::numeric_limits<float>::max();
    float end_sigma       = 0.0f;
    bool initialized      = false;
    bool initial_step     = true;
    bool skip_current_step = false;
    bool step_active      = false;
    int anchor_condition  = -1;           // (a pointer there: the first condition seen in the first active step; here its index, 0 = cond, 1 = uncond)
    bool has_diff[2]      = {false, false};  // cache_diffs: which conditions hold a stored difference
    float output_prev_norm                = 0.0f;
    bool has_prev_input                   = false;
    bool has_prev_output                  = false;
    bool has_output_prev_norm             = false;
    bool has_relative_transformation_rate = false;
    float relative_transformation_rate    = 0.0f;
    float last_input_change               = 0.0f;
    bool has_last_input_change            = false;
    int total_steps_skipped               = 0;
    int current_step_index                = -1;
    // the last decision, for the trace (not reference state)
    float trace_rate = 0.0f, trace_accumulated = 0.0f, trace_threshold = 0.0f;

    // Rule (easycache.hpp:86-98 / ucache.hpp:166-178): a percentage of the trajectory becomes a sigma through the family's t_to_sigma at timestep
    // (1 - percent) * 999; 0 % and below means "from the start" (no upper bound), 100 % and above "to the end" (sigma 0)
    static float percent_to_sigma(float percent, const std::function<float(float)>& t_to_sigma) {
        if (!t_to_sigma || percent >= 1.0f) return 0.0f;
        return percent > 0.0f ? t_to_sigma((1.0f - percent) * (TIMESTEPS - 1)) : std::numeric_limits<float>::max();
    }
    // Rule (begin_step, easycache.hpp:111-117, ucache.hpp:192-198): a step is active unless sigma > start_sigma, and unless NOT sigma > end_sigma (so a NaN is inactive)
    bool in_window(float sigma) const { return !(sigma > start_sigma) && sigma > end_sigma; }
    bool step_is_active() const { return initialized && step_active; }
    bool is_step_skipped() const { return initialized && step_active && skip_current_step; }
    bool has_cache(int cond) const { return cond >= 0 && cond < 2 && has_diff[cond]; }
    // before_condition up to the measurement (easycache.hpp:146-181, ucache.hpp:256-297), same order of tests: a new step index opens the step; outside the
    // window nothing happens; the first condition ever seen inside it becomes the anchor; in a step already decided as skipped every condition that holds a
    // difference is rebuilt from it; otherwise only the anchor, and only once it has a previous input, output and difference, is measured
    template <class Derived>
    static StepCacheAction before_condition(Derived& s, int cond, float sigma, int step_index) {
        const bool usable = s.initialized && step_index >= 0;
        if (usable && step_index != s.current_step_index) s.begin_step(step_index, sigma);
        if (!usable || !s.step_active) return SC_COMPUTE;
        if (s.initial_step) s.anchor_condition = cond, s.initial_step = false;
        if (s.skip_current_step) return s.has_cache(cond) ? SC_APPLY : SC_COMPUTE;
        const bool measurable = cond == s.anchor_condition && s.has_prev_input && s.has_prev_output && s.has_cache(cond);
        return measurable ? SC_MEASURE : SC_COMPUTE;  // (the reference's size check cannot fail here: one shape per trajectory)
    }
    // the part of after_condition both caches share once the anchor's output change is known: the new output norm, and the output-per-input change ratio when this
    // step measured an input change and both changes are positive
    void note_anchor_output(float output_change, float mean_abs) {
        has_prev_input = has_prev_output = true;
        output_prev_norm                 = mean_abs;
        has_output_prev_norm             = mean_abs > 0.0f;
        const bool both_moved            = has_last_input_change && last_input_change > 0.0f && output_change > 0.0f;
        const float ratio                = both_moved ? output_change / last_input_change : 0.0f;
        if (both_moved && std::isfinite(ratio)) relative_transformation_rate = ratio, has_relative_transformation_rate = true;
        has_last_input_change = false;
    }
    // whether a decision is due: a norm and a ratio exist and the input moved (easycache.hpp:192, ucache.hpp:309-310)
    bool can_estimate() const { return has_output_prev_norm && has_relative_transformation_rate && last_input_change > 0.0f && output_prev_norm > 0.0f; }
};

struct EasyCacheConfig {  // easycache.hpp:14-19
    bool enabled          = false;
    float reuse_threshold = 0.2f;
    float start_percent   = 0.15f;
    float end_percent     = 0.95f;
};
struct EasyCacheState : ConditionCacheState {
    EasyCacheConfig config;
    float cumulative_change_rate = 0.0f;
    // reset_runtime (easycache.hpp:50-69): every runtime field back to its default; the configuration and the sigma window stay
    void reset_runtime() {
        EasyCacheState fresh;
        fresh.config = config, fresh.initialized = initialized, fresh.start_sigma = start_sigma, fresh.end_sigma = end_sigma;
        *this = fresh;
    }
    void init(const EasyCacheConfig& cfg, const std::function<float(float)>& t_to_sigma) {  // easycache.hpp:71-80
        config      = cfg;
        initialized = cfg.enabled && (bool)t_to_sigma;
        reset_runtime();
        if (initialized) {
            start_sigma = percent_to_sigma(config.start_percent, t_to_sigma);
            end_sigma   = percent_to_sigma(config.end_percent, t_to_sigma);
        }
    }
    void begin_step(int step_index, float sigma) {  // easycache.hpp:100-118
        if (!initialized || step_index == current_step_index) return;
        current_step_index = step_index;
        skip_current_step = has_last_input_change = false;
        step_active                               = in_window(sigma);
    }
    // The rest of before_condition (easycache.hpp:182-205), given last_input_change = mean |input - prev_input| measured by the caller.  Rule: the expected relative
    // output change, ratio * input change / previous output norm, is added to the running sum; under the threshold the step is skipped (true: apply the
    // differences), otherwise the sum starts again from 0.
    bool decide(float input_change) {
        last_input_change     = input_change;
        has_last_input_change = true;
        trace_rate = trace_accumulated = trace_threshold = 0.0f;
        if (!can_estimate()) return false;
        trace_rate = (relative_transformation_rate * last_input_change) / output_prev_norm;
        cumulative_change_rate += trace_rate;
        trace_accumulated = cumulative_change_rate;
        trace_threshold   = config.reuse_threshold;
        if (!(cumulative_change_rate < config.reuse_threshold)) {
            cumulative_change_rate = 0.0f;
            return false;
        }
        skip_current_step = true;
        ++total_steps_skipped;
        return true;
    }
    // after_condition (easycache.hpp:208-258); output_change_measured = mean |output - prev_output| (counts as 0 without a previous output), mean_abs = mean |output|.
    // The caller stores the difference, prev_input and prev_output whenever the step is active.
    void after_condition(int cond, float output_change_measured, float mean_abs) {
        if (!step_is_active()) return;
        has_diff[cond] = true;
        if (cond != anchor_condition) return;
        note_anchor_output(has_prev_output ? output_change_measured : 0.0f, mean_abs);
        cumulative_change_rate = 0.0f;
    }
};

struct UCacheConfig {  // ucache.hpp:14-26
    bool enabled                = false;
    float reuse_threshold       = 1.0f;
    float start_percent         = 0.15f;
    float end_percent           = 0.95f;
    float error_decay_rate      = 1.0f;
    bool use_relative_threshold = true;
    bool adaptive_threshold     = true;
    float early_step_multiplier = 0.5f;
    float late_step_multiplier  = 1.5f;
    float relative_norm_gain    = 1.6f;
    bool reset_error_on_compute = true;
};
struct UCacheState : ConditionCacheState {
    UCacheConfig config;
    float output_change_ema         = 0.0f;
    bool has_output_change_ema      = false;
    int steps_computed_since_active = 0;
    int expected_total_steps        = 0;
    int consecutive_skipped_steps   = 0;
    float accumulated_error         = 0.0f;
    int total_active_steps          = 0;
    // (BlockMetrics, ucache.hpp:62-97, only feeds a log line there: not kept)
    // reset_runtime (ucache.hpp:100-126): every runtime field back to its default; the configuration and the sigma window stay
    void reset_runtime() {
        UCacheState fresh;
        fresh.config = config, fresh.initialized = initialized, fresh.start_sigma = start_sigma, fresh.end_sigma = end_sigma;
        *this = fresh;
    }
    void init(const UCacheConfig& cfg, const std::function<float(float)>& t_to_sigma) {  // ucache.hpp:128-137
        config      = cfg;
        initialized = cfg.enabled && (bool)t_to_sigma;
        reset_runtime();
        if (initialized) {
            start_sigma = percent_to_sigma(config.start_percent, t_to_sigma);
            end_sigma   = percent_to_sigma(config.end_percent, t_to_sigma);
        }
    }
    // Rule (ucache.hpp:139-160): the window comes from the trajectory's own ladder and overrides percent_to_sigma — the sigmas of the steps at
    // (size_t)(percent * steps), clamped to the last step, larger one first; the ladder's step count is remembered for the adaptive threshold
    void set_sigmas(const std::vector<float>& sigmas) {
        if (!initialized || sigmas.size() < 2) return;
        const size_t last    = sigmas.size() - 2;  // index of the last step
        expected_total_steps = static_cast<int>(last + 1);
        auto step_at         = [&](float percent) { return std::min(static_cast<size_t>(percent * (last + 1)), last); };
        const float a = sigmas[step_at(config.start_percent)], b = sigmas[step_at(config.end_percent)];
        start_sigma = a < b ? b : a;
        end_sigma   = a < b ? a : b;
    }
    void begin_step(int step_index, float sigma) {  // ucache.hpp:180-200
        if (!initialized || step_index == current_step_index) return;
        current_step_index = step_index;
        skip_current_step = has_last_input_change = false;
        step_active                               = in_window(sigma);
        total_active_steps += step_active ? 1 : 0;
    }
    // Rule (ucache.hpp:210-236): with the adaptive threshold on, the base threshold is halved (early_step_multiplier) while fewer than 20 % of the expected steps
    // have been computed and raised by half (late_step_multiplier) beyond 80 %; the expected count is the ladder's, or max(20, 2 * computed) when none was given
    float get_adaptive_threshold(int estimated_total_steps = 0) const {
        if (!config.adaptive_threshold) return config.reuse_threshold;
        const int total = estimated_total_steps > 0 ? estimated_total_steps : (expected_total_steps > 0 ? expected_total_steps : std::max(20, steps_computed_since_active * 2));
        const float done = std::max(0.0f, std::min(1.0f, static_cast<float>(steps_computed_since_active) / total));
        const float factor = done < 0.2f ? config.early_step_multiplier : (done > 0.8f ? config.late_step_multiplier : 1.0f);
        return config.reuse_threshold * factor;
    }
    // The rest of before_condition (ucache.hpp:299-343).  Rule: the expected output change, ratio * input change, is taken relative to sqrt(norm * dyn) when the
    // threshold is relative — norm = previous output norm, dyn = the smoothed output change * max(1, relative_norm_gain) once one exists, else norm, both floored at
    // 1e-6 — and grows by half for every step already skipped in a row; the error decays by error_decay_rate and takes the estimate on; the threshold is the
    // adaptive one, times the norm when it is absolute; under it the step is skipped, else the error is cleared if reset_error_on_compute says so.
    bool decide(float input_change) {
        last_input_change     = input_change;
        has_last_input_change = true;
        trace_rate = trace_accumulated = trace_threshold = 0.0f;
        if (!can_estimate()) return false;
        float estimate = relative_transformation_rate * last_input_change;
        if (config.use_relative_threshold) {
            const float floor_ = 1e-6f, norm = std::max(output_prev_norm, floor_);
            const float dyn    = has_output_change_ema ? std::max(output_change_ema * std::max(1.0f, config.relative_norm_gain), floor_) : norm;
            estimate           = estimate / std::sqrt(norm * dyn);
        }
        estimate *= 1.0f + 0.5f * consecutive_skipped_steps;
        accumulated_error = accumulated_error * config.error_decay_rate + estimate;
        float limit       = get_adaptive_threshold();
        if (!config.use_relative_threshold && output_prev_norm > 0.0f) limit = limit * output_prev_norm;
        trace_rate        = estimate;
        trace_accumulated = accumulated_error;
        trace_threshold   = limit;
        if (accumulated_error < limit) {
            skip_current_step = true;
            ++total_steps_skipped;
            ++consecutive_skipped_steps;
            return true;
        }
        if (config.reset_error_on_compute) accumulated_error = 0.0f;
        return false;
    }
    // after_condition (ucache.hpp:346-409): as EasyCache's, plus the count of computed steps, the end of the skip streak and the smoothed output change
    // (the first positive finite change, then 0.8 * old + 0.2 * new); the accumulated error is NOT cleared here
    void after_condition(int cond, float output_change_measured, float mean_abs) {
        if (!step_is_active()) return;
        has_diff[cond] = true;
        if (cond != anchor_condition) return;
        ++steps_computed_since_active;
        consecutive_skipped_steps = 0;
        const float moved         = has_prev_output ? output_change_measured : 0.0f;
        if (std::isfinite(moved) && moved > 0.0f) {
            output_change_ema     = has_output_change_ema ? 0.8f * output_change_ema + 0.2f * moved : moved;
            has_output_change_ema = true;
        }
        note_anchor_output(moved, mean_abs);
    }
};


// DBCacheConfig (cache_dit.hpp) restricted to what CacheDitConditionState reads on a path that changes a trajectory.  NOT kept, because they have no effect there:
// max_warmup_steps, the steps-computation mask, max_cached_steps and max_continuous_cached_steps (begin_step, cache_dit.hpp:737-760, sets step_active = true BEFORE
// it tests them and then only returns), and TaylorSeerConfig (taylor_state is updated in after_condition, :879-881, and never read)
struct CacheDitConfig {
    bool enabled                  = false;
    int Fn_compute_blocks         = 8;
    int Bn_compute_blocks         = 0;
    float residual_diff_threshold = 0.08f;
};
struct CacheDitCondState : ConditionCacheState {
    CacheDitConfig config;
    float accumulated_residual_diff = 0.0f;
    void reset_runtime() {  // cache_dit.hpp:668-681
        CacheDitCondState fresh;
        fresh.config = config, fresh.initialized = initialized, fresh.start_sigma = start_sigma, fresh.end_sigma = end_sigma;
        *this = fresh;
    }
    void init(const CacheDitConfig& cfg) {  // cache_dit.hpp:683-692
        config      = cfg;
        initialized = cfg.enabled;
        reset_runtime();
    }
    // Rule (cache_dit.hpp:694-716): the window is FIXED at 15 % .. 95 % of the ladder, whatever start_percent / end_percent say — the sigmas of the steps at
    // (size_t)(percent * n_steps), clamped to the last step, larger one first
    void set_sigmas(const std::vector<float>& sigmas) {
        if (!initialized || sigmas.size() < 2) return;
        const size_t n_steps = sigmas.size() - 1;
        const size_t a       = std::min(static_cast<size_t>(0.15f * n_steps), n_steps - 1);
        const size_t b       = std::min(static_cast<size_t>(0.95f * n_steps), n_steps - 1);
        start_sigma          = sigmas[a];
        end_sigma            = sigmas[b];
        if (start_sigma < end_sigma) std::swap(start_sigma, end_sigma);
    }
    void begin_step(int step_index, float sigma) {  // cache_dit.hpp:722-761
        if (!initialized || step_index == current_step_index) return;
        current_step_index = step_index;
        skip_current_step  = false;
        step_active        = in_window(sigma);
    }
    // Rule (cache_dit.hpp:847-857): more front blocks "computed" loosen the threshold by 2 % each around 8, back blocks tighten it by 3 % each
    float effective_threshold() const {
        float t = config.residual_diff_threshold;
        if (config.Fn_compute_blocks > 0) t *= std::max(0.5f, std::min(2.0f, 1.0f + 0.02f * (config.Fn_compute_blocks - 8)));
        if (config.Bn_compute_blocks > 0) t *= std::max(0.5f, std::min(1.0f, 1.0f - 0.03f * config.Bn_compute_blocks));
        return t;
    }
    // The rest of before_condition (cache_dit.hpp:839-870), given the two sums of calculate_residual_diff (:293-306) measured by the caller
    bool decide(float sum_diff, float sum_abs) {
        trace_rate        = sum_diff / (sum_abs + 1e-6f);
        trace_threshold   = effective_threshold();
        trace_accumulated = accumulated_residual_diff;
        if (!(trace_rate < trace_threshold)) return false;
        skip_current_step = true;
        ++total_steps_skipped;
        accumulated_residual_diff += trace_rate;
        trace_accumulated = accumulated_residual_diff;
        return true;
    }
    // after_condition (cache_dit.hpp:873-882) + update_cache (:776-795): the caller stores the difference, prev_input and prev_output of every condition; only the
    // anchor's previous input is ever read
    void after_condition(int cond) {
        if (!step_is_active()) return;
        has_diff[cond] = true;
        if (cond == anchor_condition) has_prev_input = has_prev_output = true;
    }
};

// Spectrum (src/runtime/spectrum.hpp): per denoise call, should_predict() decides from counters alone; a predicted call is a ridge-regularised Chebyshev fit through
// the last K denoised tensors, evaluated at this call's tau and blended with a first-order extrapolation; a computed call ends with update().  The tensors live
// with the loop that owns the data (a ring of K slots); this state keeps the counters, the taus of the stored calls and which slot holds which.
struct SpectrumConfig {  // spectrum.hpp:11-19
    float w            = 0.40f;
    int m              = 3;
    float lam          = 1.0f;
    int window_size    = 2;
    float flex_window  = 0.50f;
    int warmup_steps   = 4;
    float stop_percent = 0.9f;
};
struct SpectrumState {
    static constexpr int MAX_K = 16;
    SpectrumConfig config;
    int cnt                 = 0;
    int num_cached          = 0;
    float curr_ws           = 2.0f;
    int K                   = 6;
    int stop_step           = 0;
    int total_steps_skipped = 0;
    std::vector<float> T_buf;  // taus of the stored calls, oldest first (H_buf's tensors: the caller's ring)
    int head = 0;              // ring slot the next update() writes
    void init(const SpectrumConfig& cfg, size_t total_steps) {  // spectrum.hpp:33-43
        config              = cfg;
        cnt                 = 0;
        num_cached          = 0;
        curr_ws             = (float)cfg.window_size;
        K                   = std::max(cfg.m + 1, 6);
        stop_step           = (int)(cfg.stop_percent * (float)total_steps);
        total_steps_skipped = 0;
        T_buf.clear();
        head = 0;
    }
    static float taus(int step_cnt) { return (step_cnt / 50.0f) * 2.0f - 1.0f; }
    int stored() const { return (int)T_buf.size(); }
    int slot(int j) const { return ((head - stored() + j) % K + K) % K; }  // ring slot of the j-th oldest stored tensor
    bool past_warmup_before_stop() const { return cnt >= config.warmup_steps && !(stop_step > 0 && cnt >= stop_step); }
    bool should_predict() const {  // spectrum.hpp:49-59
        if (!past_warmup_before_stop() || stored() < 2) return false;
        const int ws = std::max(1, (int)std::floor(curr_ws));
        return (num_cached + 1) % ws != 0;
    }
    // update (spectrum.hpp:61-75) without the copy: returns the ring slot the caller writes `denoised` to
    int update() {
        const int at = head;
        head         = (head + 1) % K;
        T_buf.push_back(taus(cnt));
        while ((int)T_buf.size() > K) T_buf.erase(T_buf.begin());
        if (cnt >= config.warmup_steps) curr_ws += config.flex_window;
        num_cached = 0;
        cnt++;
        return at;
    }
    // The weights of predict (spectrum.hpp:79-126): Chebyshev design matrix X by recurrence at the stored taus, x* at tau_at, (XtX + lam I) v = x* through Cholesky
    // — with ONE retry after adding 1e-4 * trace / M1 to the diagonal when a pivot is not positive — and weights = X v.  f32, every operation rounded on its own.
    static void weights(const SpectrumConfig& cfg, const float* T, int k, float tau_at, float* out) {
        const int M1 = cfg.m + 1;
        std::vector<float> X((size_t)k * M1), x_star(M1), XtX((size_t)M1 * M1, 0.0f), L((size_t)M1 * M1, 0.0f), v(M1, 0.0f), y(M1, 0.0f);
        auto cheb = [M1](float t, float* row) {
            row[0] = 1.0f;
            if (M1 > 1) row[1] = t;
            for (int j = 2; j < M1; j++) row[j] = 2.0f * t * row[j - 1] - row[j - 2];
        };
        for (int i = 0; i < k; i++) cheb(T[i], &X[(size_t)i * M1]);
        cheb(tau_at, x_star.data());
        for (int i = 0; i < M1; i++)
            for (int j = 0; j < M1; j++) {
                float sum = 0.0f;
                for (int q = 0; q < k; q++) sum += X[(size_t)q * M1 + i] * X[(size_t)q * M1 + j];
                XtX[(size_t)i * M1 + j] = sum + (i == j ? cfg.lam : 0.0f);
            }
        auto cholesky = [&]() {  // spectrum.hpp:150-168; false at the first non-positive pivot (L keeps what was written until then)
            std::fill(L.begin(), L.end(), 0.0f);
            for (int i = 0; i < M1; i++)
                for (int j = 0; j <= i; j++) {
                    float sum = 0.0f;
                    for (int q = 0; q < j; q++) sum += L[(size_t)i * M1 + q] * L[(size_t)j * M1 + q];
                    if (i == j) {
                        const float diag = XtX[(size_t)i * M1 + i] - sum;
                        if (diag <= 0.0f) return false;
                        L[(size_t)i * M1 + j] = std::sqrt(diag);
                    } else {
                        L[(size_t)i * M1 + j] = (XtX[(size_t)i * M1 + j] - sum) / L[(size_t)j * M1 + j];
                    }
                }
            return true;
        };
        if (!cholesky()) {
            float trace = 0.0f;
            for (int i = 0; i < M1; i++) trace += XtX[(size_t)i * M1 + i];
            for (int i = 0; i < M1; i++) XtX[(size_t)i * M1 + i] += 1e-4f * trace / M1;
            cholesky();
        }
        for (int i = 0; i < M1; i++) {  // cholesky_solve, spectrum.hpp:170-184
            float sum = 0.0f;
            for (int j = 0; j < i; j++) sum += L[(size_t)i * M1 + j] * y[j];
            y[i] = (x_star[i] - sum) / L[(size_t)i * M1 + i];
        }
        for (int i = M1 - 1; i >= 0; i--) {
            float sum = 0.0f;
            for (int j = i + 1; j < M1; j++) sum += L[(size_t)j * M1 + i] * v[j];
            v[i] = (y[i] - sum) / L[(size_t)i * M1 + i];
        }
        for (int q = 0; q < k; q++) {
            out[q] = 0.0f;
            for (int j = 0; j < M1; j++) out[q] += X[(size_t)q * M1 + j] * v[j];
        }
    }
    // predict (spectrum.hpp:77-147) without the element loop: the weights of this call and the ring slots they go with, oldest first; then the counters
    int predict(float* w_out, int* slot_out) {
        const int k = stored();
        weights(config, T_buf.data(), k, taus(cnt), w_out);
        for (int j = 0; j < k; j++) slot_out[j] = slot(j);
        num_cached++;
        total_steps_skipped++;
        cnt++;
        return k;
    }
};
// the element loop of predict (spectrum.hpp:134-142) over ring slots `order` (oldest first) of `stride` floats each
inline void spectrum_predict_host(const float* ring, size_t stride, const int* order, int k, const float* weights, float w, size_t n, float* out) {
    const float w_taylor = 1.0f - w;
    const float *h_last = ring + (size_t)order[k - 1] * stride, *h_prev = ring + (size_t)order[k - 2] * stride;
    for (size_t f = 0; f < n; ++f) {
        float pc = 0.0f;
        for (int j = 0; j < k; ++j) {
            const float m = weights[j] * ring[(size_t)order[j] * stride + f];
            pc            = pc + m;
        }
        const float d  = h_last[f] - h_prev[f];
        const float e  = 0.5f * d;
        const float pt = h_last[f] + e;
        const float a  = w_taylor * pt;
        const float b  = w * pc;
        out[f]         = a + b;
    }
}

// SampleCacheRuntime + SampleStepCacheDispatcher (sample-cache.cpp), and the trace of include/sd-mi355x.h
struct StepCacheRuntime {
    int mode = SDM_CACHE_DISABLED;  // the CONDITION-LEVEL cache armed for this trajectory (SampleCacheMode; the three CacheDIT modes keep their own number)
    EasyCacheState easycache;
    UCacheState ucache;
    CacheDitCondState cachedit;
    SpectrumState spectrum;
    bool spectrum_enabled = false;  // SampleCacheRuntime::spectrum_enabled: beside `mode`, never together with it
    std::string status = "disabled";
    std::vector<sdm_cache_step_t> trace;
    int step_index = -1;  // of the current denoise call
    float sigma    = 0.0f;

    // Rule (sample-cache.cpp:5-15): an INFINITY threshold stands for the mode's default, 0.2 for EasyCache and 1.0 for UCache; negative thresholds count as 0
    static float get_cache_reuse_threshold(const sdm_cache_params_t& params) {
        const float mode_default = params.mode == SDM_CACHE_UCACHE ? 1.0f : 0.2f;
        const bool is_default    = params.reuse_threshold == INFINITY && (params.mode == SDM_CACHE_EASYCACHE || params.mode == SDM_CACHE_UCACHE);
        return std::max(0.0f, is_default ? mode_default : params.reuse_threshold);
    }
    // Rule (sample-cache.cpp:29-39): 0 <= start < end <= 1 (which already keeps start below 1 and end above 0; NaN fails every comparison)
    static bool has_valid_cache_percent_range(const sdm_cache_params_t& p) {
        const bool ranged = p.mode >= SDM_CACHE_EASYCACHE && p.mode <= SDM_CACHE_SPECTRUM;  // (sample-cache.cpp:185: checked in front of every mode)
        return !ranged || (p.start_percent >= 0.0f && p.start_percent < p.end_percent && p.end_percent <= 1.0f && p.start_percent < 1.0f && p.end_percent > 0.0f);
    }
    // init_sample_cache_runtime (sample-cache.cpp:176-212) with init_easycache_runtime (:41-67) / init_ucache_runtime (:69-103): the range is checked first, then
    // the family (EasyCache: DiT only, UCache: UNet only); a request that cannot be served leaves the trajectory uncached (the reference logs a warning; here
    // `status` keeps the reason).  UCache clamps error_decay_rate to [0, 1] and takes its window from the ladder.
    // The CacheDIT modes (init_cachedit_runtime, :105-146): DiT only, window from the ladder.  Spectrum (init_spectrum_runtime, :148-174): UNet and DiT alike, and
    // switched off again for the two CFG++ sample methods (stable-diffusion.cpp:2583-2590), which need an unconditional prediction a forecast does not have.
    static bool is_cachedit_mode(int m) { return m == SDM_CACHE_DBCACHE || m == SDM_CACHE_TAYLORSEER || m == SDM_CACHE_CACHE_DIT; }
    void init(const sdm_cache_params_t* params, bool is_dit, bool is_unet, const std::function<float(float)>& t_to_sigma, const std::vector<float>& sigmas,
              const sdm_cache_dit_params_t* dit_params = nullptr, const sdm_spectrum_params_t* spectrum_params = nullptr, bool method_needs_uncond = false) {
        mode = SDM_CACHE_DISABLED;
        trace.clear();
        step_index       = -1;
        easycache        = EasyCacheState();
        ucache           = UCacheState();
        cachedit         = CacheDitCondState();
        spectrum         = SpectrumState();
        spectrum_enabled = false;
        status           = "disabled";
        if (!params || params->mode == SDM_CACHE_DISABLED) return;
        const bool easy = params->mode == SDM_CACHE_EASYCACHE, dit_mode = is_cachedit_mode(params->mode), spec = params->mode == SDM_CACHE_SPECTRUM;
        if (!easy && params->mode != SDM_CACHE_UCACHE && !dit_mode && !spec)
            status = "not armed: unknown cache mode";
        else if (!has_valid_cache_percent_range(*params))
            status = "not armed: the percent range is not valid (0 <= start < end <= 1)";
        else if (dit_mode && !is_dit)
            status = "not armed: dbcache / taylorseer / cache-dit serve the DiT families only";
        else if (spec && method_needs_uncond)
            status = "not armed: spectrum does not serve the CFG++ sample methods";
        else if (!spec && !dit_mode && (easy ? !is_dit : !is_unet))
            status = easy ? "not armed: easycache serves the DiT families only" : "not armed: ucache serves the UNet families only";
        else if (!spec && !dit_mode && !t_to_sigma)
            status = "not armed: the family has no t_to_sigma";
        if (status != "disabled") return;
        if (spec) {
            SpectrumConfig config;
            if (spectrum_params)
                config = SpectrumConfig{spectrum_params->w, spectrum_params->m, spectrum_params->lam, spectrum_params->window_size, spectrum_params->flex_window,
                                        spectrum_params->warmup_steps, spectrum_params->stop_percent};
            spectrum.init(config, sigmas.size() > 0 ? sigmas.size() - 1 : 0);
            spectrum_enabled = true;
            status           = "spectrum";
            return;
        }
        if (dit_mode) {
            CacheDitConfig config;
            config.enabled = true;
            if (dit_params) config.Fn_compute_blocks = dit_params->Fn_compute_blocks, config.Bn_compute_blocks = dit_params->Bn_compute_blocks, config.residual_diff_threshold = dit_params->residual_diff_threshold;
            cachedit.init(config);
            cachedit.set_sigmas(sigmas);
            mode   = params->mode;
            status = mode == SDM_CACHE_DBCACHE ? "dbcache" : (mode == SDM_CACHE_TAYLORSEER ? "taylorseer" : "cache-dit");
            return;
        }
        const float threshold = get_cache_reuse_threshold(*params);
        if (easy) {
            EasyCacheConfig config{true, threshold, params->start_percent, params->end_percent};
            easycache.init(config, t_to_sigma);
        } else {
            UCacheConfig config;
            config.enabled = true, config.reuse_threshold = threshold;
            config.start_percent = params->start_percent, config.end_percent = params->end_percent;
            config.error_decay_rate       = std::max(0.0f, std::min(1.0f, params->error_decay_rate));
            config.use_relative_threshold = params->use_relative_threshold;
            config.reset_error_on_compute = params->reset_error_on_compute;
            ucache.init(config, t_to_sigma);
            ucache.set_sigmas(sigmas);
        }
        mode   = params->mode;
        status = easy ? "easycache" : "ucache";
    }
    bool armed() const { return mode != SDM_CACHE_DISABLED; }
    bool is_cachedit() const { return is_cachedit_mode(mode); }
    ConditionCacheState& core() { return const_cast<ConditionCacheState&>(static_cast<const StepCacheRuntime*>(this)->core()); }
    const ConditionCacheState& core() const {
        if (is_cachedit()) return cachedit;
        return mode == SDM_CACHE_UCACHE ? (const ConditionCacheState&)ucache : (const ConditionCacheState&)easycache;
    }
    int total_steps_skipped() const { return armed() ? core().total_steps_skipped : (spectrum_enabled ? spectrum.total_steps_skipped : 0); }
    // Spectrum's record of one denoise call, pushed in front of its decision; returns should_predict()
    bool spectrum_begin_call(int step, float sigma_) {
        sdm_cache_step_t r{};
        r.step    = step;
        r.sigma   = sigma_;
        r.active  = spectrum.past_warmup_before_stop();
        r.skipped = spectrum.should_predict();
        trace.push_back(r);
        return r.skipped;
    }
    bool in_window(float s) const { return armed() && core().in_window(s); }

    // SampleStepCacheDispatcher's constructor (sample-cache.cpp:214-233): one per denoise call; step is what the sampler hands the call (i + 1, negated for the
    // first stage of the two-stage methods, which therefore never sees the cache)
    void begin_call(int step, float sigma_) {
        sigma      = sigma_;
        step_index = step > 0 ? (step - 1) : -1;
        if (armed() && step_index >= 0) {
            if (mode == SDM_CACHE_EASYCACHE)
                easycache.begin_step(step_index, sigma);
            else if (mode == SDM_CACHE_UCACHE)
                ucache.begin_step(step_index, sigma);
            else
                cachedit.begin_step(step_index, sigma);
        }
        sdm_cache_step_t r{};
        r.step   = step;
        r.sigma  = sigma;
        r.active = armed() && step_index >= 0 && core().step_active;
        trace.push_back(r);
    }
    bool step_is_active() const { return armed() && step_index >= 0 && core().step_is_active(); }
    bool is_step_skipped() const { return armed() && step_index >= 0 && core().is_step_skipped(); }
    StepCacheAction before_condition(int cond) {  // sample-cache.cpp:235-254
        if (!armed() || step_index < 0) return SC_COMPUTE;
        if (is_cachedit()) return ConditionCacheState::before_condition(cachedit, cond, sigma, step_index);
        return mode == SDM_CACHE_EASYCACHE ? ConditionCacheState::before_condition(easycache, cond, sigma, step_index)
                                           : ConditionCacheState::before_condition(ucache, cond, sigma, step_index);
    }
    // the CacheDIT modes' decision from the two sums; the trace shows the relative residual diff as input_change and rate
    bool decide_rel(float sum_diff, float sum_abs, sdm_cache_step_t* rec = nullptr) {
        const bool skip     = cachedit.decide(sum_diff, sum_abs);
        sdm_cache_step_t& r = rec ? *rec : trace.back();
        r.input_change = r.rate = cachedit.trace_rate;
        r.accumulated  = cachedit.trace_accumulated;
        r.threshold    = cachedit.trace_threshold;
        r.skipped      = skip;
        return skip;
    }
    bool decide(float input_change, sdm_cache_step_t* rec = nullptr) {
        const bool skip = mode == SDM_CACHE_EASYCACHE ? easycache.decide(input_change) : ucache.decide(input_change);
        sdm_cache_step_t& r = rec ? *rec : trace.back();
        r.input_change = input_change;
        r.rate         = core().trace_rate;
        r.accumulated  = core().trace_accumulated;
        r.threshold    = core().trace_threshold;
        r.skipped      = skip;
        return skip;
    }
    // sample-cache.cpp:256-276; rec: the trace record of the step the measurements belong to (the device sampler delivers them one step late)
    void after_condition(int cond, float output_change, float mean_abs, sdm_cache_step_t* rec = nullptr) {
        if (!armed() || step_index < 0) return;
        if (is_cachedit()) return cachedit.after_condition(cond);  // (no output metrics: the trace keeps 0)
        const bool anchor = step_is_active() && cond == core().anchor_condition;
        if (anchor) {
            sdm_cache_step_t& r = rec ? *rec : trace.back();
            r.output_change     = core().has_prev_output ? output_change : 0.0f;
            r.output_norm       = mean_abs;
        }
        if (mode == SDM_CACHE_EASYCACHE)
            easycache.after_condition(cond, output_change, mean_abs);
        else
            ucache.after_condition(cond, output_change, mean_abs);
    }
};

// The three metrics exactly as the reference's loops form them: ONE float accumulator, sequential, divided by the element count
// (easycache.hpp:183-189, 226-246 / ucache.hpp:300-306, 368-396)
inline float mean_abs_diff(const float* a, const float* b, size_t ne) {
    float s = 0.0f;
    for (size_t i = 0; i < ne; ++i) s += std::fabs(a[i] - b[i]);
    if (ne > 0) s /= static_cast<float>(ne);
    return s;
}
inline float mean_abs(const float* a, size_t ne) {
    float s = 0.0f;
    for (size_t i = 0; i < ne; ++i) s += std::fabs(a[i]);
    return ne > 0 ? s / static_cast<float>(ne) : 0.0f;
}

// the host loop's arrays: prev_input / prev_output of the anchor and one diff per condition, over the whole device group
struct HostStepCacheStore {
    std::vector<float> prev_input, prev_output, diff[2];
    // store_condition_cache_diff (condition_cache_utils.hpp:10-36) + the anchor's bookkeeping of after_condition; returns through the runtime
    void after_condition(StepCacheRuntime& rt, int cond, const float* in, const float* out, size_t ne) {
        if (!rt.step_is_active()) return;
        diff[cond].resize(ne);
        for (size_t i = 0; i < ne; ++i) diff[cond][i] = out[i] - in[i];
        float output_change = 0.0f, norm = 0.0f;
        if (cond == rt.core().anchor_condition) {
            prev_input.assign(in, in + ne);
            if (!rt.is_cachedit() && rt.core().has_prev_output && prev_output.size() == ne) output_change = mean_abs_diff(out, prev_output.data(), ne);
            prev_output.assign(out, out + ne);
            if (!rt.is_cachedit()) norm = mean_abs(out, ne);
        }
        rt.after_condition(cond, output_change, norm);
    }
    // apply_condition_cache_diff (condition_cache_utils.hpp:38-60): output = input, then += diff
    void apply(int cond, const float* in, float* out, size_t ne) const {
        for (size_t i = 0; i < ne; ++i) out[i] = in[i] + diff[cond][i];
    }
    // before_condition for one condition: true = `out` was rebuilt from the cache, the forward must not run
    bool before_condition(StepCacheRuntime& rt, int cond, const float* in, float* out, size_t ne) {
        StepCacheAction a = rt.before_condition(cond);
        if (a == SC_MEASURE && rt.is_cachedit()) {  // calculate_residual_diff (cache_dit.hpp:293-306): two float accumulators, sequential
            float sum_diff = 0.0f, sum_abs = 0.0f;
            for (size_t i = 0; i < ne; ++i) sum_diff += std::fabs(prev_input[i] - in[i]), sum_abs += std::fabs(prev_input[i]);
            a = rt.decide_rel(sum_diff, sum_abs) ? SC_APPLY : SC_COMPUTE;
        } else if (a == SC_MEASURE) {
            a = rt.decide(mean_abs_diff(in, prev_input.data(), ne)) ? SC_APPLY : SC_COMPUTE;
        }
        if (a != SC_APPLY) return false;
        apply(cond, in, out, ne);
        return true;
    }
};

}  // namespace sdmi
