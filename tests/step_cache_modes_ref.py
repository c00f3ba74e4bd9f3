"""The CacheDIT modes (dbcache / taylorseer / cache-dit: one cache) and Spectrum restated in numpy float32, from the rules (not from the engine's code).

  CacheDitRef.call_arrays(step, sigma, conds)   driven by arrays: `conds` is a list of (cond_id, input, forward); the two sums are sequential float32 sums
  CacheDitRef.call_metrics(step, sigma, rec)    driven by the relative residual diff an engine trace recorded (its `rate`)
  SpectrumRef.schedule / weights / call         the counters, the ridge-regularised Chebyshev weights, and a denoise call around a `compute` callback

Every number is an np.float32 and every operation one rounded float32 operation, in the order the rules state them."""
import numpy as np

from step_cache_ref import seq_sum, valid_percent_range

F = np.float32
DBCACHE, TAYLORSEER, CACHE_DIT, SPECTRUM = 3, 4, 5, 6
NAMES = {DBCACHE: "dbcache", TAYLORSEER: "taylorseer", CACHE_DIT: "cache-dit", SPECTRUM: "spectrum"}


def clamp(v, lo, hi):
    return max(F(lo), min(F(hi), F(v)))


def effective_threshold(threshold, fn, bn):
    t = F(threshold)
    if fn > 0:
        t = F(t * clamp(F(1) + F(F(0.02) * F(fn - 8)), 0.5, 2))
    if bn > 0:
        t = F(t * clamp(F(1) - F(F(0.03) * F(bn)), 0.5, 1))
    return t


def residual_sums(prev, cur):
    prev, cur = np.asarray(prev, np.float32).ravel(), np.asarray(cur, np.float32).ravel()
    return seq_sum(np.abs(prev - cur)), seq_sum(np.abs(prev))


class CacheDitRef:
    """Window: the sigmas of steps (size_t)(0.15 n) and (size_t)(0.95 n) of the ladder, whatever the percent options say (they only have to be valid).  The first
    condition seen in an active step is the anchor.  Once the anchor has the input of a computed active step, diff = sum |prev_in - in| / (sum |prev_in| + 1e-6)
    is compared with the effective threshold; under it, every condition with a stored difference gets output = input + difference and the accumulated diff grows."""

    def __init__(self, mode, family_is_dit, sigmas, threshold=0.08, fn=8, bn=0, start_percent=0.15, end_percent=0.95):
        self.armed = False
        self.reason = "disabled"
        if not valid_percent_range(F(start_percent), F(end_percent)):
            self.reason = "invalid percent range"
            return
        if not family_is_dit:
            self.reason = "DiT families only"
            return
        self.armed, self.reason = True, NAMES[mode]
        self.threshold = effective_threshold(threshold, fn, bn)
        n = len(sigmas) - 1
        a = min(int(F(F(0.15) * F(n))), n - 1)
        b = min(int(F(F(0.95) * F(n))), n - 1)
        self.start_sigma, self.end_sigma = F(sigmas[a]), F(sigmas[b])
        if self.start_sigma < self.end_sigma:
            self.start_sigma, self.end_sigma = self.end_sigma, self.start_sigma
        self.step_index = -1
        self.active = self.skip = False
        self.anchor = None
        self.has_diff = set()
        self.has_prev = False
        self.accumulated = F(0)
        self.skipped_total = 0
        self.prev_in = None
        self.diff = {}

    def _begin(self, step, sigma):
        idx = step - 1 if step > 0 else -1
        if not self.armed or idx < 0:
            return False
        if idx != self.step_index:
            self.step_index, self.skip = idx, False
            s = F(sigma)
            self.active = (not s > self.start_sigma) and (s > self.end_sigma)
        return self.active

    def _decide(self, sum_diff=None, sum_abs=None, rate=None):
        rate = F(F(sum_diff) / F(F(sum_abs) + F(1e-6))) if rate is None else F(rate)
        skip = bool(rate < self.threshold)
        if skip:
            self.skip = True
            self.skipped_total += 1
            self.accumulated = F(self.accumulated + rate)
        return skip, rate

    def _measure_due(self, cond):
        return cond == self.anchor and not self.skip and self.has_prev

    def call_arrays(self, step, sigma, conds):
        rec = dict(step=step, sigma=F(sigma), active=False, skipped=False, rate=F(0), accumulated=F(0), threshold=F(0))
        active = rec["active"] = bool(self._begin(step, sigma))
        outs = []
        for cond, x, forward in conds:
            x = np.asarray(x, np.float32)
            if not active:
                outs.append(forward())
                continue
            if self.anchor is None:
                self.anchor = cond
            if self._measure_due(cond):
                rec["skipped"], rec["rate"] = self._decide(*residual_sums(self.prev_in, x))
                rec["accumulated"], rec["threshold"] = self.accumulated, self.threshold
            if self.skip and cond in self.has_diff:
                outs.append((x + self.diff[cond]).astype(np.float32))
                continue
            out = np.asarray(forward(), np.float32)
            self.diff[cond] = (out - x).astype(np.float32)
            self.has_diff.add(cond)
            if cond == self.anchor:
                self.prev_in, self.has_prev = x.copy(), True
            outs.append(out)
        return outs, rec

    def call_metrics(self, step, sigma, measured, n_conds=1):
        rec = dict(step=step, sigma=F(sigma), active=False, skipped=False, rate=F(0), accumulated=F(0), threshold=F(0))
        active = rec["active"] = bool(self._begin(step, sigma))
        if not active:
            return rec
        for cond in range(n_conds):
            if self.anchor is None:
                self.anchor = cond
            if self._measure_due(cond):
                rec["skipped"], rec["rate"] = self._decide(rate=measured["rate"])
                rec["accumulated"], rec["threshold"] = self.accumulated, self.threshold
            if self.skip and cond in self.has_diff:
                continue
            self.has_diff.add(cond)
            if cond == self.anchor:
                self.has_prev = True
        return rec


class SpectrumRef:
    """Per denoise call: predicted iff warm-up is over, the stop call is not reached, two tensors are stored and (num_cached + 1) % max(1, floor(window)) != 0.
    A computed call stores its denoised with tau(cnt) = cnt / 50 * 2 - 1 (at most K = max(m + 1, 6), oldest dropped), grows the window by flex_window once
    warm-up is over, and clears num_cached."""

    def __init__(self, n_steps, w=0.40, m=3, lam=1.0, window_size=2, flex_window=0.50, warmup_steps=4, stop_percent=0.9):
        self.w, self.m, self.lam, self.flex, self.warmup = F(w), int(m), F(lam), F(flex_window), int(warmup_steps)
        self.cnt = self.num_cached = self.predicted_total = 0
        self.curr_ws = F(window_size)
        self.K = max(self.m + 1, 6)
        self.stop = int(F(F(stop_percent) * F(n_steps)))
        self.H, self.T = [], []

    @staticmethod
    def tau(cnt):
        return F(F(F(F(cnt) / F(50)) * F(2)) - F(1))

    def window_open(self):
        return self.cnt >= self.warmup and not (self.stop > 0 and self.cnt >= self.stop)

    def should_predict(self):
        if not self.window_open() or len(self.T) < 2:
            return False
        return (self.num_cached + 1) % max(1, int(np.floor(self.curr_ws))) != 0

    def update(self, denoised=None):
        self.H.append(None if denoised is None else np.array(denoised, np.float32))
        self.T.append(self.tau(self.cnt))
        self.H, self.T = self.H[-self.K:], self.T[-self.K:]
        if self.cnt >= self.warmup:
            self.curr_ws = F(self.curr_ws + self.flex)
        self.num_cached = 0
        self.cnt += 1

    def note_predicted(self):
        self.num_cached += 1
        self.predicted_total += 1
        self.cnt += 1

    def schedule(self, n_calls):
        out = ""
        for _ in range(n_calls):
            if self.should_predict():
                out += "P"
                self.note_predicted()
            else:
                out += "C"
                self.update()
        return out

    @staticmethod
    def weights(taus, tau_at, m, lam):
        """Chebyshev rows by recurrence; A = XtX + lam I; Cholesky (one retry with 1e-4 * trace / M1 on the diagonal at a non-positive pivot); v; X v"""
        M1, k, lam = m + 1, len(taus), F(lam)

        def row(t):
            r = [F(1)]
            if M1 > 1:
                r.append(F(t))
            for j in range(2, M1):
                r.append(F(F(F(F(2) * F(t)) * r[j - 1]) - r[j - 2]))
            return r

        X = [row(t) for t in taus]
        xs = row(tau_at)
        A = [[F(0)] * M1 for _ in range(M1)]
        for i in range(M1):
            for j in range(M1):
                s = F(0)
                for q in range(k):
                    s = F(s + F(X[q][i] * X[q][j]))
                A[i][j] = F(s + (lam if i == j else F(0)))

        def cholesky():
            L = [[F(0)] * M1 for _ in range(M1)]
            for i in range(M1):
                for j in range(i + 1):
                    s = F(0)
                    for q in range(j):
                        s = F(s + F(L[i][q] * L[j][q]))
                    if i == j:
                        d = F(A[i][i] - s)
                        if d <= 0:
                            return L, False
                        L[i][j] = np.sqrt(d, dtype=np.float32)
                    else:
                        L[i][j] = F(F(A[i][j] - s) / L[j][j])
            return L, True

        L, ok = cholesky()
        retried = not ok
        if not ok:
            tr = F(0)
            for i in range(M1):
                tr = F(tr + A[i][i])
            for i in range(M1):
                A[i][i] = F(A[i][i] + F(F(F(1e-4) * tr) / F(M1)))
            L, _ = cholesky()
        with np.errstate(all="ignore"):
            y, v = [F(0)] * M1, [F(0)] * M1
            for i in range(M1):
                s = F(0)
                for j in range(i):
                    s = F(s + F(L[i][j] * y[j]))
                y[i] = F(F(xs[i] - s) / L[i][i])
            for i in range(M1 - 1, -1, -1):
                s = F(0)
                for j in range(i + 1, M1):
                    s = F(s + F(L[j][i] * v[j]))
                v[i] = F(F(y[i] - s) / L[i][i])
            out = np.zeros(k, np.float32)
            for q in range(k):
                s = F(0)
                for j in range(M1):
                    s = F(s + F(X[q][j] * v[j]))
                out[q] = s
        return out, retried

    @staticmethod
    def blend(hist, weights, w):
        """pc = sum oldest to newest of weights[k] * H[k]; pt = h_last + 0.5 (h_last - h_prev); out = (1 - w) pt + w pc — every operation rounded"""
        hist = [np.asarray(h, np.float32) for h in hist]
        pc = np.zeros_like(hist[0])
        for wk, h in zip(weights, hist):
            pc = pc + (F(wk) * h)
        pt = hist[-1] + (F(0.5) * (hist[-1] - hist[-2]))
        return ((F(1) - F(w)) * pt) + (F(w) * pc)

    def call(self, compute, predict=None):
        """one denoise call: -> (denoised, predicted); compute() -> denoised array; predict(hist, weights, w) replaces the numpy blend (e.g. the device kernel)"""
        if self.should_predict():
            wts, _ = self.weights(self.T, self.tau(self.cnt), self.m, self.lam)
            out = (predict or self.blend)(self.H, wts, self.w)
            self.note_predicted()
            return np.asarray(out, np.float32), True
        den = np.asarray(compute(), np.float32)
        self.update(den)
        return den, False
