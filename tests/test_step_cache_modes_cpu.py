"""The step-cache modes 3 .. 6 (dbcache / taylorseer / cache-dit: one condition-level cache of the DiT families; spectrum: a forecast of whole denoise calls, every
family) on the oracle backend: schedule and weights against the numpy restatement (tests/step_cache_modes_ref.py) bit for bit, Python-driven Euler trajectories
against the engine's host loop bit for bit, the traces, the paths that must change nothing, the requests that run uncached or are refused, Heun, and the test entry
points of the device passes on the host fallback."""
import numpy as np
import pytest

import step_cache_modes_ref as mref
import step_cache_ref as ref
from test_step_cache_cpu import FAMILIES, STEPS, conditioning, decisions, sample

F = np.float32
DIT_MODES = (mref.DBCACHE, mref.TAYLORSEER, mref.CACHE_DIT)


@pytest.fixture(scope="module")
def engines(sd, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = sd.Engine(model=getattr(sd, name), backend=oracle)
        return made[name]

    return get


def derived_dit_threshold(sd, e, name, **over):
    """1.5 x the median relative residual diff of a threshold-0 trajectory (which skips nothing and shows every step's diff)"""
    e.set_step_cache(mref.DBCACHE, cache_dit=dict(residual_diff_threshold=0.0))
    sample(sd, e, name, **over)
    rates = [r["rate"] for r in e.step_cache_trace() if r["rate"] > 0]
    assert len(rates) >= 4
    return float(1.5 * np.median(rates))


SPECTRUM_VARIANTS = [dict(), dict(window_size=1), dict(window_size=3, flex_window=0.25), dict(warmup_steps=2, stop_percent=0.75), dict(flex_window=0.0, stop_percent=1.0),
                     dict(warmup_steps=0, window_size=4, flex_window=1.5, stop_percent=0.0)]


@pytest.mark.parametrize("steps", [1, 2, 5, 8, 16, 20, 30, 60])
def test_spectrum_schedule_is_the_restatements(sd, steps):
    for over in SPECTRUM_VARIANTS:
        assert sd.spectrum_schedule(steps, **over) == mref.SpectrumRef(steps, **over).schedule(steps), (steps, over)
    if steps == 20:
        assert sd.spectrum_schedule(20) == "CCCCPCPCPPCPPCPPPCCC"
    if steps in (16, 30):
        assert sd.spectrum_schedule(steps).count("P") == {16: 6, 30: 16}[steps]


@pytest.mark.parametrize("m", [0, 1, 3, 7, 15])
def test_spectrum_weights_bit_equal(sd, m):
    K = max(m + 1, 6)
    for k in range(2, K + 1):
        for first, lam in ((4, 1.0), (0, 0.25), (9, 1e-3)):
            taus = [mref.SpectrumRef.tau(c) for c in range(first, first + 2 * k, 2)]  # every other call was computed
            at = mref.SpectrumRef.tau(first + 2 * k)
            want, _ = mref.SpectrumRef.weights(taus, at, m, lam)
            got = sd.spectrum_weights(taus, float(at), m=m, lam=lam)
            assert got.tobytes() == want.tobytes(), (m, k, lam, got, want)
    # lam = 0 with two equal taus: XtX is singular, the second pivot is not positive, the retry adds 1e-4 * trace / M1
    if m >= 1:
        taus = [F(0.3), F(0.3)]
        want, retried = mref.SpectrumRef.weights(taus, F(0.5), m, 0.0)
        assert retried
        got = sd.spectrum_weights(taus, 0.5, m=m, lam=0.0)
        assert got.tobytes() == want.tobytes(), (m, got, want)


def engine_sigmas(sd, e, name):
    """the ladder the engine samples this model on (its default scheduler), read from the trace of a cache that is armed and skips nothing"""
    e.set_step_cache(mref.SPECTRUM, spectrum=dict(warmup_steps=STEPS))
    sample(sd, e, name, cfg=1.0)
    return [F(r["sigma"]) for r in e.step_cache_trace()] + [F(0)]


def python_euler(sd, e, name, sig, cache=None, spectrum=None, predict=None):
    """sample_euler on one image with cfg = 1 over the ladder `sig`, the model through Engine.unet_forward; `cache`: a condition-level restatement around the
    forward; `spectrum`: a SpectrumRef around the whole denoise call"""
    _, dit, _, _, ch, family = FAMILIES[name]
    cond, _, y, _ = conditioning(name)
    n = ch * 8 * 8
    assert len(sig) == STEPS + 1
    x = (sd.philox_randn(11, 0, n) * F(sig[0])).astype(np.float32).reshape(1, ch, 8, 8)
    records = []
    for i in range(STEPS):
        s, s_to = F(sig[i]), F(sig[i + 1])
        c_in = F(1.0) if dit else F(1.0) / np.sqrt(s * s + F(1.0))
        t = np.array([(s if family == 2 else s * F(1000.0)) if dit else sd.lib().sd_sigma_to_t(float(s))], dtype=np.float32)  # FLUX takes sigma itself

        def denoise():
            noised = (x * c_in).astype(np.float32)
            forward = lambda: e.unet_forward(noised, t, cond, y)
            if cache is None:
                eps = forward()
            else:
                (eps,), rec = cache.call_arrays(i + 1, s, [(0, noised, forward)])
                records.append(rec)
            return eps * (-s) + x

        if spectrum is None:
            den = denoise()
        else:
            den, predicted = spectrum.call(denoise, predict)
            records.append(dict(step=i + 1, active=None, skipped=predicted))
        x = (x + (x - den) / s * (s_to - s)).astype(np.float32)
    return x, records


@pytest.mark.parametrize("name", ["SD15_TINY", "SD35_TINY"])
def test_python_driven_euler_with_spectrum_is_the_host_loop_bit_for_bit(sd, engines, name):
    e = engines(name)
    try:
        sig = engine_sigmas(sd, e, name)
        e.set_step_cache(None)
        x_off, _ = python_euler(sd, e, name, sig)
        np.testing.assert_array_equal(x_off, sample(sd, e, name, cfg=1.0))  # the driver itself is exact: whatever differs below is the cache
        for over in (dict(), dict(m=5, w=0.7, window_size=3)):
            e.set_step_cache(mref.SPECTRUM, spectrum=over)
            out = sample(sd, e, name, cfg=1.0)
            trace = e.step_cache_trace()
            x_on, records = python_euler(sd, e, name, sig, spectrum=mref.SpectrumRef(STEPS, **over))
            assert [r["skipped"] for r in records] == [r["skipped"] for r in trace] and sum(r["skipped"] for r in trace) > 0
            np.testing.assert_array_equal(x_on, out)
            assert np.abs(out - x_off).max() > 0
    finally:
        e.set_step_cache(None)


@pytest.mark.parametrize("name", ["SD35_TINY", "FLUX_TINY"])
def test_python_driven_euler_with_dbcache_is_the_host_loop_bit_for_bit(sd, engines, name):
    e = engines(name)
    try:
        sig = engine_sigmas(sd, e, name)
        e.set_step_cache(None)
        np.testing.assert_array_equal(python_euler(sd, e, name, sig)[0], sample(sd, e, name, cfg=1.0))  # the driver itself is exact
        thr = derived_dit_threshold(sd, e, name, cfg=1.0)
        e.set_step_cache(mref.DBCACHE, cache_dit=dict(residual_diff_threshold=thr))
        out = sample(sd, e, name, cfg=1.0)
        trace = e.step_cache_trace()
        x_on, records = python_euler(sd, e, name, sig, cache=mref.CacheDitRef(mref.DBCACHE, True, sig, threshold=thr))
        assert decisions(records) == decisions(trace) and sum(r["skipped"] for r in trace) > 0
        for a, b in zip(records, trace):
            for key in ("rate", "accumulated", "threshold"):
                assert F(a[key]).tobytes() == F(b[key]).tobytes(), (key, a, b)
        np.testing.assert_array_equal(x_on, out)
    finally:
        e.set_step_cache(None)


@pytest.mark.parametrize("name", ["SD35_TINY", "FLUX_TINY"])
def test_cachedit_trace_matches_the_restatement_and_the_three_modes_agree(sd, engines, name):
    e = engines(name)
    try:
        thr = derived_dit_threshold(sd, e, name)
        latents, traces = {}, {}
        for mode in DIT_MODES:
            e.set_step_cache(mode, cache_dit=dict(residual_diff_threshold=thr))
            latents[mode] = sample(sd, e, name)
            assert e.step_cache_status() == mref.NAMES[mode]
            trace = traces[mode] = e.step_cache_trace()
            assert [r["step"] for r in trace] == list(range(1, STEPS + 1))
            decided = [r for r in trace if r["threshold"] > 0]
            assert len(decided) >= 4
            for r in decided:
                assert abs(r["rate"] - r["threshold"]) > 1e-3 * r["threshold"], r
                assert r["input_change"] == r["rate"] and r["output_change"] == 0 and r["output_norm"] == 0
            r_ = mref.CacheDitRef(mode, True, [r["sigma"] for r in trace] + [0.0], threshold=thr)
            for got in trace:
                want = r_.call_metrics(got["step"], got["sigma"], got, n_conds=2)
                assert (got["active"], got["skipped"]) == (want["active"], want["skipped"]), got
                for key in ("rate", "accumulated", "threshold"):
                    assert F(got[key]).tobytes() == F(want[key]).tobytes(), (key, got, want)
            n_skipped = sum(r["skipped"] for r in trace)
            assert e.stats()["steps_skipped"] == n_skipped == r_.skipped_total and 0 < n_skipped < sum(r["active"] for r in trace)
        for mode in DIT_MODES[1:]:
            assert traces[mode] == traces[DIT_MODES[0]]
            np.testing.assert_array_equal(latents[mode], latents[DIT_MODES[0]])
        # Fn = 16 loosens the threshold by clamp(1 + 0.02 * 8) and Bn = 4 tightens it by clamp(1 - 0.03 * 4)
        e.set_step_cache(mref.CACHE_DIT, cache_dit=dict(residual_diff_threshold=thr, Fn_compute_blocks=16, Bn_compute_blocks=4))
        sample(sd, e, name)
        want = F(F(F(thr) * F(F(1) + F(F(0.02) * F(8)))) * F(F(1) - F(F(0.03) * F(4))))
        assert want == mref.effective_threshold(thr, 16, 4)
        got = {F(r["threshold"]).tobytes() for r in e.step_cache_trace() if r["threshold"] > 0}
        assert got == {want.tobytes()}
        assert mref.effective_threshold(1.0, 100, 0) == F(2) and mref.effective_threshold(1.0, 8, 40) == F(0.5) and mref.effective_threshold(1.0, 0, 0) == F(1)
    finally:
        e.set_step_cache(None)


@pytest.mark.parametrize("name", ["SD15_TINY", "SD35_TINY", "FLUX_TINY"])
def test_nothing_to_skip_and_disabling_are_bit_identical_to_no_cache(sd, oracle, engines, name):
    dit = FAMILIES[name][1]
    fresh = sd.Engine(model=getattr(sd, name), backend=oracle)  # the setter is never called on this one
    want = sample(sd, fresh, name)
    want_dev = sample(sd, fresh, name, fuse_cfg=True, device_sampler=True)
    e = engines(name)
    settings = [(mref.SPECTRUM, dict(spectrum=dict(warmup_steps=STEPS))), (mref.SPECTRUM, dict(spectrum=dict(warmup_steps=STEPS + 5)))]
    if dit:
        settings += [(mode, dict(cache_dit=dict(residual_diff_threshold=0.0))) for mode in DIT_MODES]
    try:
        for mode, kw in settings:
            e.set_step_cache(mode, **kw)
            np.testing.assert_array_equal(sample(sd, e, name), want)
            assert e.stats()["steps_skipped"] == 0 and e.step_cache_status() == mref.NAMES[mode] and len(e.step_cache_trace()) == STEPS
            np.testing.assert_array_equal(sample(sd, e, name, fuse_cfg=True, device_sampler=True), want_dev)
            assert e.stats()["steps_skipped"] == 0 and len(e.step_cache_trace()) == STEPS
            if mode != mref.SPECTRUM:
                assert sum(r["rate"] > 0 for r in e.step_cache_trace()) >= 4
            e.set_step_cache(mode)  # the defaults: (on most models) something else happens ...
            sample(sd, e, name)
            sample(sd, e, name, fuse_cfg=True, device_sampler=True)
            e.set_step_cache(ref.DISABLED)  # ... and nothing of it is left
            np.testing.assert_array_equal(sample(sd, e, name), want)
            np.testing.assert_array_equal(sample(sd, e, name, fuse_cfg=True, device_sampler=True), want_dev)
            assert e.step_cache_status() == "disabled" and e.step_cache_trace() == []
    finally:
        e.set_step_cache(None)


@pytest.mark.parametrize("name,mode", [("SD15_TINY", mref.SPECTRUM), ("SD35_TINY", mref.SPECTRUM), ("SD35_TINY", mref.DBCACHE), ("FLUX_TINY", mref.CACHE_DIT)])
def test_skipping_saves_exactly_the_skipped_forwards(sd, engines, name, mode):
    e = engines(name)
    try:
        e.set_step_cache(None)
        calls = {}
        for fuse in (False, True):
            c0 = e.stats()["unet_calls"]
            sample(sd, e, name, fuse_cfg=fuse)
            calls[fuse] = e.stats()["unet_calls"] - c0
        assert calls == {False: 2 * STEPS, True: STEPS}
        if mode == mref.SPECTRUM:
            e.set_step_cache(mode)
        else:
            thr = derived_dit_threshold(sd, e, name)
            e.set_step_cache(mode, cache_dit=dict(residual_diff_threshold=thr))
        outs, traces = {}, {}
        for fuse in (False, True):
            c0 = e.stats()["unet_calls"]
            outs[fuse] = sample(sd, e, name, fuse_cfg=fuse)
            traces[fuse] = e.step_cache_trace()
            skipped = sum(r["skipped"] for r in traces[fuse])
            assert 0 < skipped < STEPS and e.stats()["steps_skipped"] == skipped
            assert calls[fuse] - (e.stats()["unet_calls"] - c0) == skipped * (1 if fuse else 2)
            assert np.isfinite(outs[fuse]).all()
        assert decisions(traces[False]) == decisions(traces[True])
        if mode == mref.SPECTRUM:
            assert "".join("P" if r["skipped"] else "C" for r in traces[True]) == mref.SpectrumRef(STEPS).schedule(STEPS) == sd.spectrum_schedule(STEPS)
            s_ = mref.SpectrumRef(STEPS)
            for r in traces[True]:
                assert r["active"] == s_.window_open() and (r["rate"], r["accumulated"], r["threshold"], r["input_change"]) == (0, 0, 0, 0)
                s_.note_predicted() if r["skipped"] else s_.update()
        np.testing.assert_array_equal(sample(sd, e, name, fuse_cfg=True), outs[True])  # the runtime state is reset per trajectory
        np.testing.assert_array_equal(sample(sd, e, name, fuse_cfg=True, device_sampler=True), outs[True])  # on this backend the device sampler's passes are the host's
        assert decisions(e.step_cache_trace()) == decisions(traces[True]) and e.stats()["steps_skipped"] == sum(r["skipped"] for r in traces[True])
    finally:
        e.set_step_cache(None)


def test_requests_that_cannot_be_served_run_uncached_and_say_why(sd, engines):
    e = engines("SD15_TINY")
    try:
        e.set_step_cache(None)
        want = sample(sd, e, "SD15_TINY")
        for mode in DIT_MODES:  # the CacheDIT modes on a UNet family
            e.set_step_cache(mode, cache_dit=dict(residual_diff_threshold=10.0))
            np.testing.assert_array_equal(sample(sd, e, "SD15_TINY"), want)
            assert "DiT families only" in e.step_cache_status() and e.stats()["steps_skipped"] == 0
            np.testing.assert_array_equal(sample(sd, e, "SD15_TINY", device_sampler=True, fuse_cfg=True), sample(sd, e, "SD15_TINY", fuse_cfg=True))
        for method in (sd.EULER_CFG_PP, sd.EULER_A_CFG_PP):  # Spectrum with the CFG++ methods
            e.set_step_cache(None)
            want_pp = sample(sd, e, "SD15_TINY", method=method)
            e.set_step_cache(mref.SPECTRUM)
            np.testing.assert_array_equal(sample(sd, e, "SD15_TINY", method=method), want_pp)
            assert "CFG++" in e.step_cache_status() and e.stats()["steps_skipped"] == 0 and e.step_cache_trace() == []
    finally:
        e.set_step_cache(None)
    for name, mode in (("SD15_TINY", mref.SPECTRUM), ("SD35_TINY", mref.SPECTRUM), ("SD35_TINY", mref.DBCACHE), ("SD35_TINY", mref.TAYLORSEER), ("SD35_TINY", mref.CACHE_DIT)):
        e = engines(name)
        try:
            e.set_step_cache(None)
            want = sample(sd, e, name)
            for bad in (dict(start_percent=0.6, end_percent=0.4), dict(start_percent=-0.1), dict(end_percent=1.5), dict(start_percent=1.0, end_percent=1.0)):
                e.set_step_cache(mode, cache_dit=dict(residual_diff_threshold=10.0), **bad)
                np.testing.assert_array_equal(sample(sd, e, name), want)
                assert "percent range is not valid" in e.step_cache_status() and e.stats()["steps_skipped"] == 0
            if mode != mref.SPECTRUM:  # a valid range is accepted and then ignored: the window is the ladder's 15 % .. 95 %
                e.set_step_cache(mode, cache_dit=dict(residual_diff_threshold=0.0))
                sample(sd, e, name)
                window = [r["active"] for r in e.step_cache_trace()]
                e.set_step_cache(mode, cache_dit=dict(residual_diff_threshold=0.0), start_percent=0.4, end_percent=0.6)
                sample(sd, e, name)
                assert [r["active"] for r in e.step_cache_trace()] == window == [False] * 2 + [True] * 13 + [False]
        finally:
            e.set_step_cache(None)


def test_refused_parameters_and_combinations(sd, engines):
    e = engines("SD35_TINY")
    try:
        for kw in (dict(cache_dit=dict(residual_diff_threshold=float("nan"))), dict(spectrum=dict(w=float("nan"))), dict(spectrum=dict(lam=float("nan"))),
                   dict(spectrum=dict(flex_window=float("nan"))), dict(spectrum=dict(stop_percent=float("nan")))):
            with pytest.raises(sd.EngineError, match="NaN parameter"):
                e.set_step_cache(mref.SPECTRUM, **kw)
        for m in (-1, 16):
            with pytest.raises(sd.EngineError, match="0 .. 15"):
                e.set_step_cache(mref.SPECTRUM, spectrum=dict(m=m))
        e.set_step_cache(mref.SPECTRUM, spectrum=dict(m=15))
        assert np.isfinite(sample(sd, e, "SD35_TINY")).all() and e.stats()["steps_skipped"] > 0
        for mode in DIT_MODES + (mref.SPECTRUM,):
            e.set_step_cache(mode)
            for dev in (False, True):
                with pytest.raises(sd.EngineError, match="skip-layer guidance"):
                    sample(sd, e, "SD35_TINY", slg=([1], 2.0, 0.0, 1.0), device_sampler=dev, fuse_cfg=dev)
            e.set_pair_exchange(lambda ptr, count, stream: True, branch=0)
            try:
                with pytest.raises(sd.EngineError, match="CFG-pair exchange"):
                    sample(sd, e, "SD35_TINY", device_sampler=True, fuse_cfg=True)
            finally:
                e.set_pair_exchange(None)
    finally:
        e.set_pair_exchange(None)
        e.set_step_cache(None)
    e = engines("SD15_TINY")
    try:
        e.set_step_cache(mref.DBCACHE)  # not armed on this family: skip-layer parameters are ignored there as ever, and the pair exchange runs
        assert np.isfinite(sample(sd, e, "SD15_TINY")).all()
        e.set_step_cache(mref.SPECTRUM)
        e.set_pair_exchange(lambda ptr, count, stream: True, branch=0)
        with pytest.raises(sd.EngineError, match="CFG-pair exchange"):
            sample(sd, e, "SD15_TINY", device_sampler=True, fuse_cfg=True)
    finally:
        e.set_pair_exchange(None)
        e.set_step_cache(None)


def test_two_stage_method(sd, engines):
    """Heun hands the denoise call -i for the first stage and i for the second.  Spectrum counts CALLS: its schedule over the 2 * STEPS - 1 calls is the one of that
    many single-stage calls with stop_step still taken from the STEPS of the ladder.  CacheDIT never sees the negative-step stage."""
    e, name = engines("SD35_TINY"), "SD35_TINY"
    steps_seen = [s for i in range(1, STEPS) for s in (-i, i)] + [-STEPS]
    try:
        e.set_step_cache(mref.SPECTRUM)
        c0 = e.stats()["unet_calls"]
        out = sample(sd, e, name, method=sd.HEUN, fuse_cfg=True)
        trace = e.step_cache_trace()
        assert [r["step"] for r in trace] == steps_seen
        s_ = mref.SpectrumRef(STEPS)
        want = s_.schedule(len(steps_seen))
        assert "".join("P" if r["skipped"] else "C" for r in trace) == want and want != mref.SpectrumRef(len(steps_seen)).schedule(len(steps_seen))
        assert any(r["skipped"] for r in trace if r["step"] < 0) and any(r["skipped"] for r in trace if r["step"] > 0)
        assert e.stats()["unet_calls"] - c0 == want.count("C") and e.stats()["steps_skipped"] == want.count("P") and np.isfinite(out).all()

        thr = derived_dit_threshold(sd, e, name, method=sd.HEUN, fuse_cfg=True)
        e.set_step_cache(mref.DBCACHE, cache_dit=dict(residual_diff_threshold=thr))
        c0 = e.stats()["unet_calls"]
        out = sample(sd, e, name, method=sd.HEUN, fuse_cfg=True)
        trace = e.step_cache_trace()
        assert [r["step"] for r in trace] == steps_seen
        assert not any(r["active"] or r["skipped"] for r in trace if r["step"] < 0)
        skipped = sum(r["skipped"] for r in trace)
        assert 0 < skipped and e.stats()["unet_calls"] - c0 == len(trace) - skipped and np.isfinite(out).all()
    finally:
        e.set_step_cache(None)


def test_kernel_entries_on_the_host_fallback(sd, engines):
    """sd_spectrum_kernels and sd_step_cache_kernels_rel on a backend without the device passes: the host restatement (the GPU suite runs the kernels)"""
    e = engines("SD15_TINY")
    assert not e.step_cache_device_passes()
    rng = np.random.default_rng(3)
    for n, k in ((1, 2), (5, 3), (1027, 6), (4 * 16 * 16, 16)):
        hist = rng.standard_normal((k, n)).astype(np.float32)
        hist[:, 1::3] = 0.0
        weights = (rng.standard_normal(k) * 2).astype(np.float32)
        got = e.spectrum_kernels(hist, weights, 0.4)
        np.testing.assert_array_equal(got, mref.SpectrumRef.blend(list(hist), weights, 0.4))
        a, pi = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        sums = e.step_cache_kernels_rel(a, pi, c_in=0.75)
        want = [np.abs((a * F(0.75)).astype(np.float32) - pi).sum(dtype=np.float64), np.abs(pi).sum(dtype=np.float64)]
        np.testing.assert_allclose(sums, want, rtol=max(n * 2.0**-24, 1e-7))
        assert e.step_cache_kernels_rel(pi, pi, c_in=1.0)[0] == 0
