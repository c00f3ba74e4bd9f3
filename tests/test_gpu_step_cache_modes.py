"""The step-cache modes 3 .. 6 on the MI355X backend: Spectrum's forecast pass and the CacheDIT modes' probe (kernels/step_cache.hip) against numpy, the
device-resident sampler with Spectrum / DBCache armed against the host loop on the same backend, a Python-driven trajectory through the forecast kernel, plan
reuse and a run on poisoned buffers.  With SDCPP_GPU_TESTS_ON_ORACLE=1 both sides run the CPU oracle and the device sampler takes its host restatements."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import step_cache_modes_ref as mref

pytestmark = pytest.mark.gpu
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"
STEPS = 16
F = np.float32
MODELS = {  # name -> (context shape, y width, latent channels, is DiT, takes sigma as its timestep)
    "SD15_TINY": ((1, 77, 64), None, 4, False, False),
    "SD35_TINY": ((1, 40, 96), 64, 16, True, False),
    "FLUX_TINY": ((1, 24, 96), 64, 16, True, True),
}
SIZES = [1, 3, 255, 256, 1027, 4 * 16 * 16, 2**20 + 3]


@pytest.fixture(scope="module")
def engines(sd, gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = sd.Engine(model=getattr(sd, name), backend=gpu, flash_attn=True)
        return made[name]

    return get


@pytest.mark.parametrize("k", [2, 6, 16])
@pytest.mark.parametrize("n", SIZES)
def test_spectrum_predict_pass(sd, engines, n, k):
    """Bit-equal to the numpy rule (every operation rounded to f32 on its own, oldest to newest) and run-to-run identical.  The entry point pushes every tensor
    into its ring slot the way the sampler does and rotates the slots, so the slot order the kernel is handed is not the storage order.  n = 1, 3: the scalar tail
    alone; 255, 1027, 2^20 + 3: quads plus a tail; 2^20 + 3: more quads than the grid has threads."""
    e = engines("SD15_TINY")
    assert e.step_cache_device_passes() == ON_GPU, "on the MI355X backend the passes are its HIP kernels, never the host restatement"
    rng = np.random.default_rng(1000 * k + n % 997)
    hist = rng.standard_normal((k, n)).astype(np.float32)
    hist[:, 1::3] = 0.0  # exact zeros (from n = 2 on) ...
    hist[k - 1, ::7] = 0.0
    weights = (rng.standard_normal(k) * 1.5).astype(np.float32)
    weights[0], weights[-1] = F(-2.25), F(3.5)  # mixed sign, magnitudes above 1
    for w in (0.4, 1.0):
        got = e.spectrum_kernels(hist, weights, w)
        np.testing.assert_array_equal(got, mref.SpectrumRef.blend(list(hist), weights, w))
        assert e.spectrum_kernels(hist, weights, w).tobytes() == got.tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_probe_rel_pass(sd, engines, n):
    """Every term is non-negative, so a summation tree at most 128 additions deep is within 128 * 2^-24 = 7.6e-6 < 1e-5 of the exact sum, relatively (the
    oracle-side restatement adds sequentially: n * 2^-24).  in == prev_in gives exactly 0; run-to-run bit-identical."""
    e = engines("SD15_TINY")
    rng = np.random.default_rng(n)
    a, pi = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    a[1::3] = 0.0
    pi[2::5] = 0.0
    c_in = F(0.4371)
    sums = e.step_cache_kernels_rel(a, pi, c_in=c_in)
    want = [np.abs((a * c_in).astype(np.float32) - pi).sum(dtype=np.float64), np.abs(pi).sum(dtype=np.float64)]
    bound = 1e-5 if ON_GPU else max(1e-5, n * 2.0**-24)
    rel = [abs(float(s) - w) / w if w > 0 else abs(float(s)) for s, w in zip(sums, want)]
    print(f"n {n}: relative error of the sums {rel[0]:.2e} {rel[1]:.2e} (bound {bound:.1e})")
    assert max(rel) <= bound
    assert e.step_cache_kernels_rel(a, pi, c_in=c_in).tobytes() == sums.tobytes()
    same = e.step_cache_kernels_rel(pi, pi, c_in=1.0)
    assert same[0] == 0.0 and (abs(float(same[1]) - want[1]) / want[1] <= bound if want[1] > 0 else same[1] == 0.0)


def conditioning(name):
    cshape, ydim = MODELS[name][:2]
    rng = np.random.default_rng(5)
    cond, uncond = rng.standard_normal(cshape).astype(np.float32), rng.standard_normal(cshape).astype(np.float32)
    y = None if ydim is None else rng.standard_normal((1, ydim)).astype(np.float32)
    uy = None if ydim is None else rng.standard_normal((1, ydim)).astype(np.float32)
    return cond, uncond, y, uy


def sample(sd, e, name, **over):
    cond, uncond, y, uy = conditioning(name)
    kw = dict(width=64, height=64, steps=STEPS, cfg=4.0, seed=11, batch=1, method=sd.EULER, cond_y=y, uncond_y=uy, fuse_cfg=True)
    kw.update(over)
    return e.sample_latents(cond, uncond if kw["cfg"] != 1.0 else None, **kw)


def derived_threshold(sd, e, name, **over):
    """1.5 x the median relative residual diff of a threshold-0 trajectory of the host loop (see tests/test_step_cache_modes_cpu.py)"""
    e.set_step_cache(mref.DBCACHE, cache_dit=dict(residual_diff_threshold=0.0))
    sample(sd, e, name, **over)
    rates = [r["rate"] for r in e.step_cache_trace() if r["rate"] > 0]
    assert len(rates) >= 4
    return float(1.5 * np.median(rates))


def decisions(trace):
    return [(r["step"], r["active"], r["skipped"]) for r in trace]


def spectrum_decisions(steps):
    """the (step, active, skipped) list of a single-stage trajectory under the default Spectrum options, from the restatement"""
    s_, out = mref.SpectrumRef(steps), []
    for i in range(steps):
        predicted = s_.should_predict()
        out.append((i + 1, s_.window_open(), predicted))
        s_.note_predicted() if predicted else s_.update()
    return out


CASES = [("SD15_TINY", "spectrum"), ("SD35_TINY", "spectrum"), ("SD35_TINY", "dbcache"), ("FLUX_TINY", "dbcache")]
# Spectrum, diff / base of every case below measured on the oracle backend (SDCPP_GPU_TESTS_ON_ORACLE=1), where the device sampler's forecast and ring are the host
# restatement and its graphs run the same node kernels as the host loop's forward: base = 0 and diff = 0 in all 8 Spectrum cases, so the largest measured ratio is
# 0 (taken as 0 / 0 = 0) and the factor is max(2, 2 * 0) = 2.  On the MI355X (profiles/step_cache_modes_gpu.txt) base and diff are 0 in all 8 cases as well: the
# forecast kernel gives the host loop's bits and the step graph's tail rounds like the host loop's update.
SPECTRUM_FACTOR = 2.0


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("method", ["EULER", "EULER_A"])
@pytest.mark.parametrize("name,cache", CASES)
def test_device_sampler_against_the_host_loop(sd, engines, name, cache, method, batch):
    """Same decisions / schedule, finite latents, and max |dev - host| <= factor x base with base the same difference with the cache off; equal when base is 0.
    DBCache: factor 2, the sibling test's rule (the skipped steps replay stored differences, they do not amplify).  Spectrum: SPECTRUM_FACTOR, see above."""
    e = engines(name)
    over = dict(method=getattr(sd, method), batch=batch, device_batch=batch)
    try:
        e.set_step_cache(None)
        base = float(np.abs(sample(sd, e, name, device_sampler=True, **over) - sample(sd, e, name, **over)).max())
        if cache == "spectrum":
            e.set_step_cache(mref.SPECTRUM)
            factor = SPECTRUM_FACTOR
        else:
            thr = derived_threshold(sd, e, name, **over)
            e.set_step_cache(mref.DBCACHE, cache_dit=dict(residual_diff_threshold=thr))
            factor = 2.0
        host = sample(sd, e, name, **over)
        t_host, n_host = e.step_cache_trace(), e.stats()["steps_skipped"]
        if cache == "spectrum":
            assert "".join("P" if r["skipped"] else "C" for r in t_host) == sd.spectrum_schedule(STEPS)
        else:
            decided = [r for r in t_host if r["threshold"] > 0]
            assert len(decided) >= 4
            for r in decided:  # what makes "identical decisions" a fair demand on two summation orders
                assert abs(r["rate"] - r["threshold"]) > 1e-3 * r["threshold"], f"step {r['step']} decides within 1e-3 of its threshold"
        assert n_host > 0
        dev = sample(sd, e, name, device_sampler=True, **over)
        assert decisions(e.step_cache_trace()) == decisions(t_host) and e.stats()["steps_skipped"] == n_host
        diff = float(np.abs(dev - host).max())
        print(f"{name} {cache} {method} batch {batch}: device vs host max |diff| cache off {base:.3e}, cache on {diff:.3e}, ratio {diff / base if base > 0 else 0.0:.3f}; "
              f"{n_host} steps skipped")
        assert np.isfinite(dev).all()
        assert diff <= factor * base if base > 0 else diff == 0
    finally:
        e.set_step_cache(None)


def test_python_driven_euler_through_the_forecast_kernel(sd, engines):
    """cfg 1, one image: the model through Engine.unet_forward on this backend, Spectrum through the restatement with sd_spectrum_kernels as its element loop —
    the bits of the backend's host loop, whose forecast is the host's element loop."""
    e, name = engines("SD15_TINY"), "SD15_TINY"
    cond, _, y, _ = conditioning(name)
    ch = MODELS[name][2]
    try:
        e.set_step_cache(mref.SPECTRUM)
        out = sample(sd, e, name, cfg=1.0, fuse_cfg=False)
        trace = e.step_cache_trace()
        sig = [F(r["sigma"]) for r in trace] + [F(0)]
        spectrum = mref.SpectrumRef(STEPS)
        x = (sd.philox_randn(11, 0, ch * 64) * sig[0]).astype(np.float32).reshape(1, ch, 8, 8)
        predicted = []
        for i in range(STEPS):
            s, s_to = sig[i], sig[i + 1]
            c_in = F(1.0) / np.sqrt(s * s + F(1.0))
            t = np.array([sd.lib().sd_sigma_to_t(float(s))], dtype=np.float32)
            compute = lambda: e.unet_forward((x * c_in).astype(np.float32), t, cond, y) * (-s) + x
            kernel = lambda hist, wts, w: e.spectrum_kernels(np.stack([h.ravel() for h in hist]), wts, w).reshape(x.shape)
            den, p = spectrum.call(compute, kernel)
            predicted.append(p)
            x = (x + (x - den) / s * (s_to - s)).astype(np.float32)
        assert predicted == [bool(r["skipped"]) for r in trace] and sum(predicted) == 6
        np.testing.assert_array_equal(x, out)
    finally:
        e.set_step_cache(None)


@pytest.mark.parametrize("name,cache", [("SD15_TINY", "spectrum"), ("SD35_TINY", "dbcache")])
def test_second_call_replays_its_graphs(sd, engines, name, cache):
    e = engines(name)
    try:
        if cache == "spectrum":
            e.set_step_cache(mref.SPECTRUM)
        else:
            e.set_step_cache(mref.DBCACHE, cache_dit=dict(residual_diff_threshold=derived_threshold(sd, e, name)))
        first = sample(sd, e, name, device_sampler=True)
        trace = e.step_cache_trace()
        skipped = sum(r["skipped"] for r in trace)
        if cache == "spectrum":  # the recording graph (calls that can still feed a forecast), the predicted-step graph and the plain graph (from the stop call on) all ran
            assert 0 < skipped < STEPS - skipped and not trace[-1]["active"] and not trace[-1]["skipped"]
        else:
            assert 0 < skipped < sum(r["active"] for r in trace) < STEPS
        s0 = sd.backend_stats() if ON_GPU else None
        second = sample(sd, e, name, device_sampler=True)
        np.testing.assert_array_equal(second, first)
        assert decisions(e.step_cache_trace()) == decisions(trace)
        if ON_GPU:
            s1 = sd.backend_stats()
            print("second call:", {k: s1[k] - s0[k] for k in ("graphs_computed", "plans_built", "graph_replays")})
            assert s1["plans_built"] == s0["plans_built"] and s1["graphs_computed"] - s0["graphs_computed"] == STEPS
    finally:
        e.set_step_cache(None)


POISON_CHILD = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
import numpy as np
import sdcpp_amd as sd
import step_cache_modes_ref as mref
import test_gpu_step_cache_modes as t
sd.lib()
if t.ON_GPU:
    sd.load_mi355x_backend()
    backend = "MI355X0"
else:
    sd.load_backend({root!r} + "/oracle/_build/libggml-cpu-oracle.so")
    backend = "CPU-oracle"
for name, cache in (("SD15_TINY", "spectrum"), ("SD35_TINY", "spectrum"), ("SD35_TINY", "dbcache")):
    e = sd.Engine(model=getattr(sd, name), backend=backend, flash_attn=True)
    if cache == "spectrum":
        e.set_step_cache(mref.SPECTRUM)
    else:
        e.set_step_cache(mref.DBCACHE, cache_dit=dict(residual_diff_threshold={thr}))
    out = t.sample(sd, e, name, device_sampler=True, method=sd.EULER_A)
    print(name, cache, "FINITE" if np.isfinite(out).all() else "NOT FINITE", "DECISIONS", t.decisions(e.step_cache_trace()))
"""


def test_device_path_on_poisoned_buffers(sd, engines):
    """GGML_MI355X_POISON=1 fills every fresh device buffer with NaN patterns: a pass or a graph that read a ring slot, spectrum.denoised, prev_in, the differences
    or a sum before anything wrote it would turn the latents NaN or change a decision"""
    want = {}
    e = engines("SD35_TINY")
    try:
        thr = derived_threshold(sd, e, "SD35_TINY", method=sd.EULER_A)
        e.set_step_cache(mref.DBCACHE, cache_dit=dict(residual_diff_threshold=thr))
        sample(sd, e, "SD35_TINY", device_sampler=True, method=sd.EULER_A)
        want[("SD35_TINY", "dbcache")] = decisions(e.step_cache_trace())
        assert any(s for _, _, s in want[("SD35_TINY", "dbcache")])
    finally:
        e.set_step_cache(None)
    for name in ("SD15_TINY", "SD35_TINY"):
        want[(name, "spectrum")] = spectrum_decisions(STEPS)
    root = str(Path(__file__).resolve().parent.parent)
    env = dict(os.environ, GGML_MI355X_POISON="1")
    r = subprocess.run([sys.executable, "-c", POISON_CHILD.format(root=root, thr=repr(thr))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "NOT FINITE" not in r.stdout and r.stdout.count("FINITE") == 3
    for (name, cache), dec in want.items():
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith(name + " " + cache))
        assert line.endswith("DECISIONS " + str(dec)), (line, dec)
