"""Step caches on the MI355X backend: the probe / record passes (kernels/step_cache.hip) against numpy, and the device-resident sampler with a cache armed against
the host loop on the same backend — same decisions, latents as close as the two paths are without a cache — plus plan reuse and a run on poisoned buffers.
With SDCPP_GPU_TESTS_ON_ORACLE=1 both sides run the CPU oracle and the device sampler takes its host restatement of the two passes."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import step_cache_ref as ref

pytestmark = pytest.mark.gpu
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"
STEPS = 16
MODELS = {  # name -> (mode, context shape, y width)
    "SD15_TINY": (ref.UCACHE, (1, 77, 64), None),
    "SD35_TINY": (ref.EASYCACHE, (1, 40, 96), 64),
    "FLUX_TINY": (ref.EASYCACHE, (1, 24, 96), 64),
}


@pytest.fixture(scope="module")
def engines(sd, gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = sd.Engine(model=getattr(sd, name), backend=gpu, flash_attn=True)
        return made[name]

    return get


@pytest.mark.parametrize("n", [1, 3, 255, 256, 1027, 4 * 16 * 16, 2**20 + 3])
def test_probe_and_record_passes(sd, engines, n):
    """diff / prev_in / prev_out bit-equal to numpy float32.  The sums: every term is non-negative, so a summation tree at most 128 additions deep is within
    128 * 2^-24 = 7.6e-6 < 1e-5 of the exact sum, relatively (the kernels' depth is 86; the oracle-side restatement adds sequentially: count * 2^-24).  Exact zeros,
    in == prev_in (the sum is exactly 0), a prev_out that was never written, and run-to-run bit-identical sums."""
    e = engines("SD15_TINY")
    e.set_step_cache(ref.UCACHE)
    assert e.step_cache_device_passes() == ON_GPU, "on the MI355X backend the two passes are its HIP kernels, never the host restatement"
    try:
        rng = np.random.default_rng(n)
        for k in (1, 2):
            for nb in (1, 3):
                a, pi, po = (rng.standard_normal((nb, n)).astype(np.float32) for _ in range(3))
                o = rng.standard_normal((nb, k, n)).astype(np.float32)
                a[:, 1::3] = 0.0   # exact zeros in every operand (from n = 3 on)
                o[:, :, 2::5] = 0.0
                po[:, 1::2] = 0.0
                c_in = np.float32(0.4371)
                stats, diff, pin2, pout2 = e.step_cache_kernels(a, o, pi, po, c_in=c_in)
                np.testing.assert_array_equal(diff, o - a[:, None, :])
                np.testing.assert_array_equal(pin2, a)
                np.testing.assert_array_equal(pout2, o[:, 0, :])
                want = [np.abs((a * c_in).astype(np.float32) - pi).sum(dtype=np.float64), np.abs(o[:, 0, :] - po).sum(dtype=np.float64), np.abs(o[:, 0, :]).sum(dtype=np.float64)]
                bound = 1e-5 if ON_GPU else max(1e-5, n * nb * 2.0**-24)
                rel = [abs(float(s) - w) / w if w > 0 else abs(float(s)) for s, w in zip(stats, want)]
                print(f"n {n} k {k} nb {nb}: relative error of the sums {rel[0]:.2e} {rel[1]:.2e} {rel[2]:.2e} (bound {bound:.1e})")
                assert max(rel) <= bound
                again = e.step_cache_kernels(a, o, pi, po, c_in=c_in)[0]
                assert again.tobytes() == stats.tobytes()
                s_same = e.step_cache_kernels(a, o, a, None, c_in=1.0)[0]  # in == prev_in, and no previous output
                assert s_same[0] == 0.0 and s_same[1] == 0.0 and abs(float(s_same[2]) - want[2]) / want[2] <= bound
    finally:
        e.set_step_cache(None)


def sample(sd, e, name, **over):
    _, cshape, ydim = MODELS[name]
    rng = np.random.default_rng(5)
    cond, uncond = rng.standard_normal(cshape).astype(np.float32), rng.standard_normal(cshape).astype(np.float32)
    y = None if ydim is None else rng.standard_normal((1, ydim)).astype(np.float32)
    uy = None if ydim is None else rng.standard_normal((1, ydim)).astype(np.float32)
    kw = dict(width=64, height=64, steps=STEPS, cfg=4.0, seed=11, batch=1, method=sd.EULER, cond_y=y, uncond_y=uy, fuse_cfg=True)
    kw.update(over)
    return e.sample_latents(cond, uncond, **kw)


def derived_threshold(sd, e, name, **over):
    """1.5 x the median per-step rate of a threshold-0 trajectory of the host loop (see tests/test_step_cache_cpu.py)"""
    e.set_step_cache(MODELS[name][0], reuse_threshold=0.0)
    sample(sd, e, name, **over)
    rates = [r["rate"] for r in e.step_cache_trace() if r["rate"] > 0]
    assert len(rates) >= 4
    return float(1.5 * np.median(rates))


def decisions(trace):
    return [(r["step"], r["active"], r["skipped"]) for r in trace]


# seeds chosen (on the oracle backend) so that no decision of the host trace sits within 1e-3 of its threshold
SEEDS = {("SD15_TINY", "EULER", 1): 11, ("SD15_TINY", "EULER", 2): 11, ("SD15_TINY", "EULER_A", 1): 11, ("SD15_TINY", "EULER_A", 2): 11,
         ("SD35_TINY", "EULER", 1): 11, ("SD35_TINY", "EULER", 2): 11, ("SD35_TINY", "EULER_A", 1): 11, ("SD35_TINY", "EULER_A", 2): 11,
         ("FLUX_TINY", "EULER", 1): 15, ("FLUX_TINY", "EULER", 2): 16, ("FLUX_TINY", "EULER_A", 1): 11, ("FLUX_TINY", "EULER_A", 2): 11}


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("method", ["EULER", "EULER_A"])
@pytest.mark.parametrize("name", ["SD15_TINY", "SD35_TINY", "FLUX_TINY"])
def test_device_sampler_decides_like_the_host_loop(sd, engines, name, method, batch):
    e = engines(name)
    mode = MODELS[name][0]
    over = dict(method=getattr(sd, method), batch=batch, device_batch=batch, seed=SEEDS[(name, method, batch)])
    try:
        thr = derived_threshold(sd, e, name, **over)
        e.set_step_cache(None)
        base = float(np.abs(sample(sd, e, name, device_sampler=True, **over) - sample(sd, e, name, **over)).max())
        e.set_step_cache(mode, reuse_threshold=thr)
        host = sample(sd, e, name, **over)
        t_host = e.step_cache_trace()
        decided = [r for r in t_host if r["threshold"] > 0]
        assert sum(r["skipped"] for r in t_host) > 0 and len(decided) >= 4
        for r in decided:  # what makes "identical decisions" a fair demand on two summation orders
            assert abs(r["accumulated"] - r["threshold"]) > 1e-3 * r["threshold"], f"step {r['step']} decides within 1e-3 of its threshold: choose another seed"
        dev = sample(sd, e, name, device_sampler=True, **over)
        t_dev = e.step_cache_trace()
        assert decisions(t_dev) == decisions(t_host)
        diff = float(np.abs(dev - host).max())
        print(f"{name} {method} batch {batch}: device vs host max |diff| cache off {base:.3e}, cache on {diff:.3e}; {sum(r['skipped'] for r in t_host)} steps skipped")
        assert np.isfinite(dev).all()
        assert diff <= 2 * base if base > 0 else diff == 0
    finally:
        e.set_step_cache(None)


@pytest.mark.parametrize("name", ["SD15_TINY", "SD35_TINY"])
def test_threshold_zero_on_the_device_path_changes_nothing(sd, engines, name):
    """probe, read-back, the recording graph and the record pass run on every active step, nothing is skipped: the latents are the uncached device path's bits"""
    e = engines(name)
    try:
        for over in (dict(), dict(method=sd.EULER_A, batch=2, device_batch=2), dict(cfg=1.0)):
            e.set_step_cache(None)
            want = sample(sd, e, name, device_sampler=True, **over)
            e.set_step_cache(MODELS[name][0], reuse_threshold=0.0)
            got = sample(sd, e, name, device_sampler=True, **over)
            trace = e.step_cache_trace()
            assert e.stats()["steps_skipped"] == 0 and sum(r["active"] for r in trace) >= 10 and sum(r["rate"] > 0 for r in trace) >= 4
            np.testing.assert_array_equal(got, want)
    finally:
        e.set_step_cache(None)


def test_second_call_replays_the_recording_and_skip_graphs(sd, engines):
    e, name = engines("SD15_TINY"), "SD15_TINY"
    try:
        thr = derived_threshold(sd, e, name)
        e.set_step_cache(ref.UCACHE, reuse_threshold=thr)
        first = sample(sd, e, name, device_sampler=True)
        trace = e.step_cache_trace()
        assert 0 < sum(r["skipped"] for r in trace) < sum(r["active"] for r in trace) < STEPS  # all three graphs ran
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
import test_gpu_step_cache as t
sd.lib()
if t.ON_GPU:
    sd.load_mi355x_backend()
    backend = "MI355X0"
else:
    sd.load_backend({root!r} + "/oracle/_build/libggml-cpu-oracle.so")
    backend = "CPU-oracle"
for name in ("SD15_TINY", "SD35_TINY"):
    e = sd.Engine(model=getattr(sd, name), backend=backend, flash_attn=True)
    e.set_step_cache(t.MODELS[name][0], reuse_threshold={thr}[name])
    out = t.sample(sd, e, name, device_sampler=True, method=sd.EULER_A)
    print(name, "FINITE" if np.isfinite(out).all() else "NOT FINITE", "DECISIONS", t.decisions(e.step_cache_trace()))
"""


def test_device_path_on_poisoned_buffers(sd, engines):
    """GGML_MI355X_POISON=1 fills every fresh device buffer with NaN patterns: a pass or a graph that read prev_out / diff / the sums before anything wrote them
    would turn the latents NaN or change a decision"""
    thr, want = {}, {}
    for name in ("SD15_TINY", "SD35_TINY"):
        e = engines(name)
        try:
            thr[name] = derived_threshold(sd, e, name, method=sd.EULER_A)
            e.set_step_cache(MODELS[name][0], reuse_threshold=thr[name])
            sample(sd, e, name, device_sampler=True, method=sd.EULER_A)
            want[name] = decisions(e.step_cache_trace())
            assert any(s for _, _, s in want[name])
        finally:
            e.set_step_cache(None)
    root = str(Path(__file__).resolve().parent.parent)
    env = dict(os.environ, GGML_MI355X_POISON="1")
    r = subprocess.run([sys.executable, "-c", POISON_CHILD.format(root=root, thr=repr(thr))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "NOT FINITE" not in r.stdout and r.stdout.count("FINITE") == 2
    for name in want:
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith(name))
        assert line.endswith("DECISIONS " + str(want[name])), (line, want[name])
