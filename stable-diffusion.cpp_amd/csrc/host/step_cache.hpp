// step_cache.hpp — the reference's condition-level step caches, restated on the host: EasyCache (DiT families; src/runtime/easycache.hpp) and UCache (UNet
// families; src/runtime/ucache.hpp), their set-up (src/runtime/sample-cache.cpp:5-103, 176-212) and the per-step dispatcher (sample-cache.cpp:214-291) the
// denoise call wraps around every model forward (src/stable-diffusion.cpp:2688, 2779-2795, 2817).
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
// Out of scope: DBCache / TaylorSeer / CacheDIT (src/runtime/cache_dit.hpp) and Spectrum reach into the model's blocks.
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

// SampleCacheRuntime + SampleStepCacheDispatcher (sample-cache.cpp) for the two modes, and the trace of include/sd-mi355x.h
struct StepCacheRuntime {
    int mode = SDM_CACHE_DISABLED;  // what is ARMED for this trajectory (SampleCacheMode)
    EasyCacheState easycache;
    UCacheState ucache;
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
        const bool ranged = p.mode == SDM_CACHE_EASYCACHE || p.mode == SDM_CACHE_UCACHE;
        return !ranged || (p.start_percent >= 0.0f && p.start_percent < p.end_percent && p.end_percent <= 1.0f && p.start_percent < 1.0f && p.end_percent > 0.0f);
    }
    // init_sample_cache_runtime (sample-cache.cpp:176-212) with init_easycache_runtime (:41-67) / init_ucache_runtime (:69-103): the range is checked first, then
    // the family (EasyCache: DiT only, UCache: UNet only); a request that cannot be served leaves the trajectory uncached (the reference logs a warning; here
    // `status` keeps the reason).  UCache clamps error_decay_rate to [0, 1] and takes its window from the ladder.
    void init(const sdm_cache_params_t* params, bool is_dit, bool is_unet, const std::function<float(float)>& t_to_sigma, const std::vector<float>& sigmas) {
        mode = SDM_CACHE_DISABLED;
        trace.clear();
        step_index = -1;
        easycache  = EasyCacheState();
        ucache     = UCacheState();
        status     = "disabled";
        if (!params || params->mode == SDM_CACHE_DISABLED) return;
        const bool easy = params->mode == SDM_CACHE_EASYCACHE;
        if (!easy && params->mode != SDM_CACHE_UCACHE)
            status = "not armed: unknown cache mode";
        else if (!has_valid_cache_percent_range(*params))
            status = "not armed: the percent range is not valid (0 <= start < end <= 1)";
        else if (easy ? !is_dit : !is_unet)
            status = easy ? "not armed: easycache serves the DiT families only" : "not armed: ucache serves the UNet families only";
        else if (!t_to_sigma)
            status = "not armed: the family has no t_to_sigma";
        if (status != "disabled") return;
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
    ConditionCacheState& core() { return mode == SDM_CACHE_UCACHE ? (ConditionCacheState&)ucache : (ConditionCacheState&)easycache; }
    const ConditionCacheState& core() const { return mode == SDM_CACHE_UCACHE ? (const ConditionCacheState&)ucache : (const ConditionCacheState&)easycache; }
    int total_steps_skipped() const { return armed() ? core().total_steps_skipped : 0; }
    bool in_window(float s) const { return armed() && core().in_window(s); }

    // SampleStepCacheDispatcher's constructor (sample-cache.cpp:214-233): one per denoise call; step is what the sampler hands the call (i + 1, negated for the
    // first stage of the two-stage methods, which therefore never sees the cache)
    void begin_call(int step, float sigma_) {
        sigma      = sigma_;
        step_index = step > 0 ? (step - 1) : -1;
        if (armed() && step_index >= 0) {
            if (mode == SDM_CACHE_EASYCACHE)
                easycache.begin_step(step_index, sigma);
            else
                ucache.begin_step(step_index, sigma);
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
        return mode == SDM_CACHE_EASYCACHE ? ConditionCacheState::before_condition(easycache, cond, sigma, step_index)
                                           : ConditionCacheState::before_condition(ucache, cond, sigma, step_index);
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
            if (rt.core().has_prev_output && prev_output.size() == ne) output_change = mean_abs_diff(out, prev_output.data(), ne);
            prev_output.assign(out, out + ne);
            norm = mean_abs(out, ne);
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
        if (a == SC_MEASURE) a = rt.decide(mean_abs_diff(in, prev_input.data(), ne)) ? SC_APPLY : SC_COMPUTE;
        if (a != SC_APPLY) return false;
        apply(cond, in, out, ne);
        return true;
    }
};

}  // namespace sdmi
