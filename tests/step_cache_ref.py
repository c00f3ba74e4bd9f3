"""EasyCache and UCache restated in numpy float32, from the rules (not from the engine's code): the window in sigma, the anchor, the three means, the
accumulated estimate against the threshold.  Two ways in:

  StepCacheRef.call_arrays(step, sigma, conds)   driven by arrays: `conds` is a list of (cond_id, input, forward) — the means are sequential float32 sums
  StepCacheRef.call_metrics(step, sigma, rec)    driven by the metrics an engine trace recorded (input_change / output_change / output_norm)

Every number is an np.float32 and every operation one rounded float32 operation, in the order the rules state them."""
import numpy as np

F = np.float32
TIMESTEPS = 1000
DISABLED, EASYCACHE, UCACHE = 0, 1, 2
FLT_MAX = np.finfo(np.float32).max


def seq_sum(a):
    """one float32 accumulator, sequential"""
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    return np.add.accumulate(a, dtype=np.float32)[-1] if a.size else F(0)


def mean_abs_diff(a, b):
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    return F(seq_sum(np.abs(a - b)) / F(a.size))


def mean_abs(a):
    a = np.asarray(a, np.float32).ravel()
    return F(seq_sum(np.abs(a)) / F(a.size))


def valid_percent_range(start, end):
    return 0.0 <= start < 1.0 and 0.0 < end <= 1.0 and start < end


class StepCacheRef:
    def __init__(self, mode, family_is_dit, sigmas, t_to_sigma, reuse_threshold=float("inf"), start_percent=0.15, end_percent=0.95, error_decay_rate=1.0,
                 use_relative_threshold=True, reset_error_on_compute=True):
        self.mode = DISABLED
        self.reason = "disabled"
        if mode == DISABLED:
            return
        if not valid_percent_range(F(start_percent), F(end_percent)):
            self.reason = "invalid percent range"
            return
        if (mode == EASYCACHE) != bool(family_is_dit):
            self.reason = "mode does not fit the model family"
            return
        self.mode = mode
        self.reason = "easycache" if mode == EASYCACHE else "ucache"
        thr = F(reuse_threshold)
        if np.isposinf(thr):
            thr = F(0.2) if mode == EASYCACHE else F(1.0)
        self.threshold = max(F(0), thr)
        self.decay = min(F(1), max(F(0), F(error_decay_rate)))
        self.relative = bool(use_relative_threshold)
        self.reset_on_compute = bool(reset_error_on_compute)

        def percent_to_sigma(p):
            p = F(p)
            if p <= 0:
                return FLT_MAX
            if p >= 1:
                return F(0)
            return F(t_to_sigma(float((F(1) - p) * F(TIMESTEPS - 1))))

        self.start_sigma, self.end_sigma = percent_to_sigma(start_percent), percent_to_sigma(end_percent)
        self.expected_total = 0
        if mode == UCACHE and len(sigmas) >= 2:  # the window comes from the ladder itself
            n = len(sigmas) - 1
            self.expected_total = n
            a = min(int(F(F(start_percent) * F(n))), n - 1)
            b = min(int(F(F(end_percent) * F(n))), n - 1)
            self.start_sigma, self.end_sigma = F(sigmas[a]), F(sigmas[b])
            if self.start_sigma < self.end_sigma:
                self.start_sigma, self.end_sigma = self.end_sigma, self.start_sigma
        # runtime
        self.step_index = -1
        self.active = False
        self.skip = False
        self.anchor = None
        self.has_diff = set()
        self.has_prev_in = self.has_prev_out = False
        self.prev_norm = F(0)
        self.rate = None            # output change per input change of the last computed step that had both
        self.last_in_change = None  # this step's, once measured
        self.accumulated = F(0)
        self.ema = None
        self.computed = 0
        self.consecutive = 0
        self.skipped_total = 0
        # arrays (array-driven entry)
        self.prev_in = self.prev_out = None
        self.diff = {}

    # ---- shared pieces -------------------------------------------------------------------------------------------------------------------
    def _begin(self, step, sigma):
        idx = step - 1 if step > 0 else -1
        self.call_index = idx
        if self.mode == DISABLED or idx < 0:
            return False
        if idx != self.step_index:
            self.step_index = idx
            self.skip = False
            self.last_in_change = None
            s = F(sigma)
            self.active = (not s > self.start_sigma) and (s > self.end_sigma)
        return self.active

    def _adaptive_threshold(self):
        total = self.expected_total if self.expected_total > 0 else max(20, self.computed * 2)
        progress = min(F(1), max(F(0), F(F(self.computed) / F(total))))
        mult = F(0.5) if progress < F(0.2) else (F(1.5) if progress > F(0.8) else F(1))
        return F(self.threshold * mult)

    def _decide(self, in_change):
        """-> (skip, rate, accumulated, threshold) with the numbers as they stand right after the update"""
        in_change = F(in_change)
        self.last_in_change = in_change
        if self.rate is None or not (self.prev_norm > 0) or not (in_change > 0):
            return False, F(0), F(0), F(0)
        if self.mode == EASYCACHE:
            est = F(F(self.rate * in_change) / self.prev_norm)
            self.accumulated = F(self.accumulated + est)
            acc, thr = self.accumulated, self.threshold
            skip = bool(acc < thr)
            if not skip:
                self.accumulated = F(0)
        else:
            est = F(self.rate * in_change)
            if self.relative:
                base = max(self.prev_norm, F(1e-6))
                dyn = max(F(self.ema * max(F(1), F(1.6))), F(1e-6)) if self.ema is not None else base
                est = F(est / np.sqrt(F(base * dyn), dtype=np.float32))
            est = F(est * F(F(1) + F(F(0.5) * F(self.consecutive))))
            self.accumulated = F(F(self.accumulated * self.decay) + est)
            thr = self._adaptive_threshold()
            if not self.relative and self.prev_norm > 0:
                thr = F(thr * self.prev_norm)
            acc = self.accumulated
            skip = bool(acc < thr)
            if skip:
                self.consecutive += 1
            elif self.reset_on_compute:
                self.accumulated = F(0)
        if skip:
            self.skip = True
            self.skipped_total += 1
        return skip, est, acc, thr

    def _after_anchor(self, out_change, norm):
        out_change = F(out_change) if self.has_prev_out else F(0)
        if self.mode == UCACHE:
            self.computed += 1
            self.consecutive = 0
            if np.isfinite(out_change) and out_change > 0:
                self.ema = out_change if self.ema is None else F(F(F(0.8) * self.ema) + F(F(0.2) * out_change))
        self.has_prev_in = self.has_prev_out = True
        self.prev_norm = F(norm)
        if self.last_in_change is not None and self.last_in_change > 0 and out_change > 0:
            r = F(out_change / self.last_in_change)
            if np.isfinite(r):
                self.rate = r
        if self.mode == EASYCACHE:
            self.accumulated = F(0)
        self.last_in_change = None
        return out_change

    def _wants_measurement(self, cond):
        return cond == self.anchor and not self.skip and self.has_prev_in and self.has_prev_out and cond in self.has_diff

    # ---- driven by arrays ----------------------------------------------------------------------------------------------------------------
    def call_arrays(self, step, sigma, conds):
        """conds: [(cond_id, input array, forward() -> output array)], in evaluation order.  Returns (outputs list, record dict)."""
        rec = dict(step=step, sigma=F(sigma), active=False, skipped=False, input_change=F(0), output_change=F(0), output_norm=F(0), rate=F(0), accumulated=F(0), threshold=F(0))
        active = self._begin(step, sigma)
        rec["active"] = bool(active)
        outs = []
        for cond, x, forward in conds:
            x = np.asarray(x, np.float32)
            if not active:
                outs.append(forward())
                continue
            if self.anchor is None:
                self.anchor = cond
            if self._wants_measurement(cond):
                m = mean_abs_diff(x, self.prev_in)
                skip, rec["rate"], rec["accumulated"], rec["threshold"] = self._decide(m)
                rec["input_change"], rec["skipped"] = m, skip
            if self.skip and cond in self.has_diff:
                outs.append((x + self.diff[cond]).astype(np.float32))
                continue
            out = np.asarray(forward(), np.float32)
            self.diff[cond] = (out - x).astype(np.float32)
            self.has_diff.add(cond)
            if cond == self.anchor:
                oc = mean_abs_diff(out, self.prev_out) if self.has_prev_out else F(0)
                norm = mean_abs(out)
                rec["output_change"], rec["output_norm"] = self._after_anchor(oc, norm), norm
                self.prev_in, self.prev_out = x.copy(), out.copy()
            outs.append(out)
        return outs, rec

    # ---- driven by measured metrics ----------------------------------------------------------------------------------------------------
    def call_metrics(self, step, sigma, measured, n_conds=1):
        """measured: a trace record of the engine (its input_change / output_change / output_norm are used where the rules measure them).  Returns the record
        the rules produce."""
        rec = dict(step=step, sigma=F(sigma), active=False, skipped=False, rate=F(0), accumulated=F(0), threshold=F(0))
        active = self._begin(step, sigma)
        rec["active"] = bool(active)
        if not active:
            return rec
        for cond in range(n_conds):
            if self.anchor is None:
                self.anchor = cond
            if self._wants_measurement(cond):
                rec["skipped"], rec["rate"], rec["accumulated"], rec["threshold"] = self._decide(measured["input_change"])
            if self.skip and cond in self.has_diff:
                continue
            self.has_diff.add(cond)
            if cond == self.anchor:
                self._after_anchor(measured["output_change"], measured["output_norm"])
        return rec
