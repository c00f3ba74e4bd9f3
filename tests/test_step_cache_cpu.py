"""Step caches (sd_set_step_cache: EasyCache on the DiT families, UCache on the UNet families) on the oracle backend: the host state machines against the numpy
restatement (tests/step_cache_ref.py) bit for bit, a Python-driven Euler trajectory against the engine's host loop, the off / threshold-0 paths against an engine that
never heard of the cache, the refusals, and the guidance / sampler / batching modes around it.  Every test calls set_step_cache."""
import numpy as np
import pytest

import step_cache_ref as ref

STEPS = 16
# model -> (cache mode that fits it, is DiT, context shape, y width or None, latent channels, denoiser family of get_sigmas_sched)
FAMILIES = {
    "SD15_TINY": (ref.UCACHE, False, (1, 77, 64), None, 4, 0),
    "SDXL_TINY": (ref.UCACHE, False, (1, 77, 64), 96, 4, 0),
    "SD35_TINY": (ref.EASYCACHE, True, (1, 40, 96), 64, 16, 1),
    "FLUX_TINY": (ref.EASYCACHE, True, (1, 24, 96), 64, 16, 2),
}


@pytest.fixture(scope="module")
def engines(sd, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = sd.Engine(model=getattr(sd, name), backend=oracle)
        return made[name]

    return get


def conditioning(name, seed=5):
    _, _, cshape, ydim, _, _ = FAMILIES[name]
    rng = np.random.default_rng(seed)
    cond, uncond = rng.standard_normal(cshape).astype(np.float32), rng.standard_normal(cshape).astype(np.float32)
    y = None if ydim is None else rng.standard_normal((1, ydim)).astype(np.float32)
    uy = None if ydim is None else rng.standard_normal((1, ydim)).astype(np.float32)
    return cond, uncond, y, uy


def sample(sd, e, name, cfg=4.0, size=64, **over):
    cond, uncond, y, uy = conditioning(name)
    kw = dict(width=size, height=size, steps=STEPS, cfg=cfg, seed=11, batch=1, method=sd.EULER, cond_y=y, uncond_y=uy)
    kw.update(over)
    return e.sample_latents(cond, uncond if kw["cfg"] != 1.0 else None, **kw)


def derived_threshold(sd, e, name, factor=1.5, cache_kw=None, key="rate", **over):
    """A threshold taken from what the model does, not from the outcome: with threshold 0 nothing is skipped and the trace shows every step's estimated rate;
    `factor` x their median lets roughly the calmer half of the steps through.  (UCache scales its threshold by 0.5 .. 1.5 along the trajectory.)  key =
    "accumulated": for UCache without the reset on compute, where the error of the computed steps keeps adding up and the threshold has to be taken from that sum."""
    mode = FAMILIES[name][0]
    e.set_step_cache(mode, reuse_threshold=0.0, **(cache_kw or {}))
    sample(sd, e, name, **over)
    rates = [r[key] for r in e.step_cache_trace() if r["rate"] > 0]
    assert len(rates) >= 4, "the trace of an armed cache shows the per-step rates"
    return float(factor * np.median(rates))


def decisions(trace):
    return [(r["step"], r["active"], r["skipped"]) for r in trace]


@pytest.mark.parametrize("name,cache_kw", [
    ("SD15_TINY", {}),
    ("SD15_TINY", dict(use_relative_threshold=False)),
    ("SD15_TINY", dict(reset_error_on_compute=False, error_decay_rate=0.9)),
    ("SDXL_TINY", dict(start_percent=0.1, end_percent=0.8)),
    ("SD35_TINY", {}),
    ("FLUX_TINY", dict(start_percent=0.05, end_percent=0.9)),
])
def test_state_machine_matches_the_restatement_bit_for_bit(sd, engines, name, cache_kw):
    """The engine's trace carries the three measured means of every step; the restatement, fed those, must reach the same active / skipped flags and the same
    accumulated value and effective threshold, bit for bit."""
    e = engines(name)
    mode, dit = FAMILIES[name][:2]
    try:
        thr = derived_threshold(sd, e, name, cache_kw=cache_kw, key="rate" if cache_kw.get("reset_error_on_compute", True) else "accumulated")
        for threshold in (0.0, thr):
            e.set_step_cache(mode, reuse_threshold=threshold, **cache_kw)
            sample(sd, e, name)
            assert e.step_cache_status() == ("easycache" if dit else "ucache")
            trace = e.step_cache_trace()
            assert len(trace) == STEPS and [r["step"] for r in trace] == list(range(1, STEPS + 1))
            sigmas = [r["sigma"] for r in trace] + [0.0]
            r_ = ref.StepCacheRef(mode, dit, sigmas, e.t_to_sigma, reuse_threshold=threshold, **cache_kw)
            n_skipped = 0
            for got in trace:
                want = r_.call_metrics(got["step"], got["sigma"], got, n_conds=2)
                assert (got["active"], got["skipped"]) == (want["active"], want["skipped"]), got
                for key in ("rate", "accumulated", "threshold"):
                    assert np.float32(got[key]).tobytes() == np.float32(want[key]).tobytes(), (key, got, want)
                n_skipped += got["skipped"]
            assert e.stats()["steps_skipped"] == n_skipped == r_.skipped_total
            assert (n_skipped > 0) == (threshold > 0)
    finally:
        e.set_step_cache(None)


def python_euler(sd, e, name, cache):
    """sample_euler on one image with cfg = 1, the model through Engine.unet_forward, the cache through the array-driven restatement"""
    _, dit, _, _, ch, family = FAMILIES[name]
    cond, _, y, _ = conditioning(name)
    n = ch * 8 * 8
    sig = sd.get_sigmas_sched(family, sd.SCHED_DISCRETE, STEPS)
    x = (sd.philox_randn(11, 0, n) * np.float32(sig[0])).astype(np.float32).reshape(1, ch, 8, 8)
    records = []
    for i in range(STEPS):
        s, s_to = np.float32(sig[i]), np.float32(sig[i + 1])
        c_in = np.float32(1.0) if dit else np.float32(1.0) / np.sqrt(s * s + np.float32(1.0))
        t = np.array([s * np.float32(1000.0) if dit else sd.lib().sd_sigma_to_t(float(s))], dtype=np.float32)
        noised = (x * c_in).astype(np.float32)
        forward = lambda: e.unet_forward(noised, t, cond, y)
        if cache is None:
            eps = forward()
        else:
            (eps,), rec = cache.call_arrays(i + 1, s, [(0, noised, forward)])
            records.append(rec)
        den = eps * (-s) + x
        x = (x + (x - den) / s * (s_to - s)).astype(np.float32)
    return x, records, sig


@pytest.mark.parametrize("name", ["SD15_TINY", "SD35_TINY"])
def test_python_driven_euler_trajectory(sd, engines, name):
    """Decisions identical; the latents differ from the engine's by no more than twice what the same driver differs with the cache off (the two sides contract
    multiply-adds differently; equal when that baseline is 0)."""
    e = engines(name)
    mode, dit = FAMILIES[name][:2]
    try:
        thr = derived_threshold(sd, e, name, cfg=1.0)
        e.set_step_cache(None)
        x_off, _, sig = python_euler(sd, e, name, None)
        base = float(np.abs(x_off - sample(sd, e, name, cfg=1.0)).max())
        e.set_step_cache(mode, reuse_threshold=thr)
        out = sample(sd, e, name, cfg=1.0)
        trace = e.step_cache_trace()
        x_on, records, _ = python_euler(sd, e, name, ref.StepCacheRef(mode, dit, list(sig), e.t_to_sigma, reuse_threshold=thr))
        assert decisions(records) == decisions(trace)
        assert 0 < sum(r["skipped"] for r in trace)
        diff = float(np.abs(x_on - out).max())
        print(f"{name}: driver vs engine max |diff| cache off {base:.3e}, cache on {diff:.3e}")
        assert diff <= 2 * base if base > 0 else diff == 0
    finally:
        e.set_step_cache(None)


@pytest.mark.parametrize("name", ["SD15_TINY", "FLUX_TINY"])
def test_threshold_zero_and_disabling_are_bit_identical_to_no_cache(sd, oracle, engines, name):
    mode = FAMILIES[name][0]
    fresh = sd.Engine(model=getattr(sd, name), backend=oracle)  # the setter is never called on this one
    want = sample(sd, fresh, name)
    want_dev = sample(sd, fresh, name, fuse_cfg=True, device_sampler=True)
    assert fresh.step_cache_trace() == [] and fresh.stats()["steps_skipped"] == 0
    e = engines(name)
    try:
        e.set_step_cache(mode, reuse_threshold=0.0)
        np.testing.assert_array_equal(sample(sd, e, name), want)
        assert e.stats()["steps_skipped"] == 0 and any(r["active"] for r in e.step_cache_trace())
        np.testing.assert_array_equal(sample(sd, e, name, fuse_cfg=True, device_sampler=True), want_dev)
        assert e.stats()["steps_skipped"] == 0 and any(r["active"] for r in e.step_cache_trace())
        e.set_step_cache(mode)  # the default threshold: something else happens ...
        sample(sd, e, name)
        e.set_step_cache(ref.DISABLED)  # ... and nothing of it is left
        np.testing.assert_array_equal(sample(sd, e, name), want)
        np.testing.assert_array_equal(sample(sd, e, name, fuse_cfg=True, device_sampler=True), want_dev)
        assert e.step_cache_status() == "disabled" and e.step_cache_trace() == []
    finally:
        e.set_step_cache(None)


def test_requests_that_cannot_be_served_run_uncached_and_say_why(sd, engines):
    for name, wrong in (("SD15_TINY", ref.EASYCACHE), ("SD35_TINY", ref.UCACHE)):
        e = engines(name)
        try:
            e.set_step_cache(None)
            want = sample(sd, e, name)
            e.set_step_cache(wrong, reuse_threshold=10.0)
            np.testing.assert_array_equal(sample(sd, e, name), want)
            assert "families only" in e.step_cache_status() and e.stats()["steps_skipped"] == 0
            for bad in (dict(start_percent=0.6, end_percent=0.4), dict(start_percent=-0.1), dict(end_percent=1.5), dict(start_percent=1.0, end_percent=1.0)):
                e.set_step_cache(FAMILIES[name][0], reuse_threshold=10.0, **bad)
                np.testing.assert_array_equal(sample(sd, e, name), want)
                np.testing.assert_array_equal(sample(sd, e, name, device_sampler=True, fuse_cfg=True), sample(sd, e, name, fuse_cfg=True))
                assert "percent range is not valid" in e.step_cache_status() and e.stats()["steps_skipped"] == 0
        finally:
            e.set_step_cache(None)


def test_refused_combinations(sd, engines):
    e = engines("SD35_TINY")
    try:
        e.set_step_cache(ref.EASYCACHE)
        for dev in (False, True):
            with pytest.raises(sd.EngineError, match="skip-layer guidance"):
                sample(sd, e, "SD35_TINY", slg=([1], 2.0, 0.0, 1.0), device_sampler=dev, fuse_cfg=dev)
        e.set_step_cache(ref.UCACHE)  # not armed on this family: skip-layer guidance runs as ever
        assert np.isfinite(sample(sd, e, "SD35_TINY", slg=([1], 2.0, 0.0, 1.0))).all()
    finally:
        e.set_step_cache(None)
    e = engines("SD15_TINY")
    try:
        e.set_step_cache(ref.UCACHE)
        e.set_pair_exchange(lambda ptr, count, stream: True, branch=0)
        with pytest.raises(sd.EngineError, match="CFG-pair exchange"):
            sample(sd, e, "SD15_TINY", device_sampler=True, fuse_cfg=True)
    finally:
        e.set_pair_exchange(None)
        e.set_step_cache(None)


@pytest.mark.parametrize("name", ["SD15_TINY", "SDXL_TINY", "SD35_TINY", "FLUX_TINY"])
def test_skipping_saves_exactly_the_skipped_forwards(sd, engines, name):
    """0 < skipped < active under the derived threshold; the model runs exactly that many times less; fused and separate CFG forwards decide alike; a second
    trajectory on the same context repeats the first (the runtime state is reset per trajectory)."""
    e = engines(name)
    mode = FAMILIES[name][0]
    try:
        thr = derived_threshold(sd, e, name)
        e.set_step_cache(None)
        calls = {}
        for fuse in (False, True):
            c0 = e.stats()["unet_calls"]
            sample(sd, e, name, fuse_cfg=fuse)
            calls[fuse] = e.stats()["unet_calls"] - c0
        assert calls == {False: 2 * STEPS, True: STEPS}
        e.set_step_cache(mode, reuse_threshold=thr)
        outs, traces = {}, {}
        for fuse in (False, True):
            c0 = e.stats()["unet_calls"]
            outs[fuse] = sample(sd, e, name, fuse_cfg=fuse)
            traces[fuse] = e.step_cache_trace()
            skipped = sum(r["skipped"] for r in traces[fuse])
            active = sum(r["active"] for r in traces[fuse])
            print(f"{name} fuse={fuse}: {skipped} of {active} active steps skipped, threshold {thr:.4g}")
            assert 0 < skipped < active and e.stats()["steps_skipped"] == skipped
            assert calls[fuse] - (e.stats()["unet_calls"] - c0) == skipped * (1 if fuse else 2)
            assert np.isfinite(outs[fuse]).all()
        assert decisions(traces[False]) == decisions(traces[True])
        np.testing.assert_array_equal(sample(sd, e, name, fuse_cfg=True), outs[True])
        assert decisions(e.step_cache_trace()) == decisions(traces[True])
    finally:
        e.set_step_cache(None)


def test_two_stage_method_never_caches_its_first_stage(sd, engines):
    """Heun: the first stage of a step arrives with a negated step number and is always computed; the second stage is the one the cache sees."""
    e, name = engines("SD15_TINY"), "SD15_TINY"
    try:
        thr = derived_threshold(sd, e, name, method=sd.HEUN, factor=2.5)
        e.set_step_cache(ref.UCACHE, reuse_threshold=thr)
        c0 = e.stats()["unet_calls"]
        out = sample(sd, e, name, method=sd.HEUN, fuse_cfg=True)
        trace = e.step_cache_trace()
        assert [r["step"] for r in trace] == [s for i in range(1, STEPS) for s in (-i, i)] + [-STEPS]
        assert not any(r["active"] or r["skipped"] for r in trace if r["step"] < 0)
        skipped = sum(r["skipped"] for r in trace)
        print(f"Heun: {skipped} second stages skipped")
        assert 0 < skipped and e.stats()["unet_calls"] - c0 == len(trace) - skipped and np.isfinite(out).all()
        sigmas = sorted({r["sigma"] for r in trace}, reverse=True) + [0.0]
        r_ = ref.StepCacheRef(ref.UCACHE, False, sigmas, e.t_to_sigma, reuse_threshold=thr)
        for got in trace:
            want = r_.call_metrics(got["step"], got["sigma"], got, n_conds=2)
            assert (got["active"], got["skipped"], np.float32(got["accumulated"]).tobytes()) == (want["active"], want["skipped"], np.float32(want["accumulated"]).tobytes())
    finally:
        e.set_step_cache(None)


@pytest.mark.parametrize("name", ["SD15_TINY", "SD35_TINY"])
def test_euler_a_and_device_groups(sd, engines, name):
    """Euler-A: a skipped step still draws (and on the device path uploads) its ancestral noise, so the Philox order is the uncached one — the device-resident
    sampler, whose sums on this backend are the host's, gives the host loop's bits with the same decisions.  device_batch 2: one decision per group over both
    images, repeated by the device path."""
    e = engines(name)
    mode = FAMILIES[name][0]
    try:
        for over in (dict(method=sd.EULER_A), dict(method=sd.EULER_A, batch=2, device_batch=2), dict(method=sd.EULER, batch=3, device_batch=2)):
            thr = derived_threshold(sd, e, name, fuse_cfg=True, **over)
            e.set_step_cache(mode, reuse_threshold=thr)
            host = sample(sd, e, name, fuse_cfg=True, **over)
            t_host, n_host = e.step_cache_trace(), e.stats()["steps_skipped"]
            dev = sample(sd, e, name, fuse_cfg=True, device_sampler=True, **over)
            t_dev = e.step_cache_trace()
            assert decisions(t_dev) == decisions(t_host) and e.stats()["steps_skipped"] == n_host
            assert sum(r["skipped"] for r in t_host) > 0
            np.testing.assert_array_equal(dev, host)
            for a, b in zip(t_dev, t_host):  # the device path books a step's output sums one step late: the trace still shows them on their own step
                assert (a["input_change"], a["output_change"], a["output_norm"], a["accumulated"]) == (b["input_change"], b["output_change"], b["output_norm"], b["accumulated"])
    finally:
        e.set_step_cache(None)


def test_kernel_entry_on_the_host_fallback(sd, engines):
    """sd_step_cache_kernels on a backend without the device passes: the host restatement of the same quantities (the GPU suite runs the kernels)"""
    e = engines("SD15_TINY")
    e.set_step_cache(ref.UCACHE)
    try:
        rng = np.random.default_rng(3)
        for nb, k, n in ((1, 1, 5), (3, 2, 1027)):
            a, pi, po = (rng.standard_normal((nb, n)).astype(np.float32) for _ in range(3))
            o = rng.standard_normal((nb, k, n)).astype(np.float32)
            stats, diff, pin2, pout2 = e.step_cache_kernels(a, o, pi, po, c_in=0.75)
            np.testing.assert_array_equal(diff, o - a[:, None, :])
            np.testing.assert_array_equal(pin2, a)
            np.testing.assert_array_equal(pout2, o[:, 0, :])
            want = [np.abs(a * np.float32(0.75) - pi).sum(dtype=np.float64), np.abs(o[:, 0, :] - po).sum(dtype=np.float64), np.abs(o[:, 0, :]).sum(dtype=np.float64)]
            np.testing.assert_allclose(stats, want, rtol=n * nb * 2.0**-24)
            assert e.step_cache_kernels(a, o, pi, None)[0][1] == 0
    finally:
        e.set_step_cache(None)
