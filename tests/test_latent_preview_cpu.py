"""Latent previews while sampling (sdm_set_preview_callback; csrc/host/preview.hpp) on the oracle backend, where the byte stages are the host restatement: the two
passes against the numpy rules (tests/latent_preview_ref.py) byte for byte, the family tables against bytes the reference's own preview_latent_video produced
(tests/golden/latent_preview.npz), the callback sequence of host-loop and device-sampler trajectories against the schedule rule, the paths that must change
nothing, and the refusals."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import latent_preview_ref as ref
from latent_preview_ref import STEPS, Recorder, sample

F = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden" / "latent_preview.npz"
# (W, H, C, N): the shapes of the device tests (tests/test_gpu_latent_preview.py)
SHAPES = [(5, 3, 4, 1), (8, 8, 16, 3), (33, 17, 16, 2), (64, 64, 4, 2), (128, 128, 16, 1), (8, 8, 3, 2), (8, 8, 128, 1)]
HEUN_STEPS = [s for i in range(1, STEPS + 1) for s in ((-i, i) if i < STEPS else (-i,))]  # the second stage of the last step is not run (sigma 0)


@pytest.fixture(scope="module")
def engines(sd, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = sd.Engine(model=getattr(sd, name), backend=oracle)
        return made[name]

    return get


def custom_table(c, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((c, 3)) * (0.6 / np.sqrt(c))).astype(F), (rng.standard_normal(3) * 0.05).astype(F)


@pytest.mark.parametrize("shape", SHAPES)
def test_latent_preview_pass_equals_the_restatement(sd, engines, shape):
    """NaN, +-inf, -0.0 and exact zeros sit in the input; about a third of the pixels clamp at each end"""
    w, h, c, n = shape
    e = engines("SD15_TINY")
    assert not e.preview_device_passes()  # the oracle backend has no exports: this is the host restatement
    proj, bias = (None, None) if c == 3 else custom_table(c, c)
    try:
        e.set_preview_projection(proj, bias)
        x = ref.make_latent((n, c, h, w), 7 * w + c, proj)
        for in_scale in (1.0, 0.4371):
            got = e.latent_preview(x, in_scale)
            want = ref.latent_preview(x, proj, bias, in_scale)
            assert got.shape == (n, h, w, 3)
            np.testing.assert_array_equal(got, want)
            lo, hi = float((want == 0).mean()), float((want == 255).mean())
            if in_scale == 1.0 and w * h >= 64:
                assert 0.2 < lo < 0.45 and 0.2 < hi < 0.45, (lo, hi)
    finally:
        e.set_preview_projection(None)


@pytest.mark.parametrize("shape", [(5, 3, 1), (64, 64, 2), (67, 31, 3)])
def test_planar_to_u8_pass_equals_the_restatement(sd, engines, shape):
    """values <= 0, >= 1, every k / 255 and (k + 0.5) / 255 with their two f32 neighbours; and the existing host conversion gives the same bytes"""
    w, h, n = shape
    e = engines("SD15_TINY")
    x = ref.make_image((n, 3, h, w), w)
    got = e.planar_to_u8(x)
    np.testing.assert_array_equal(got, ref.planar_to_u8(x))
    one = np.empty((h, w, 3), dtype=np.uint8)
    sd.lib().sd_planar_rgb_to_u8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    sd.lib().sd_planar_rgb_to_u8.restype = None
    sd.lib().sd_planar_rgb_to_u8(x[0].ctypes.data_as(C.c_void_p), w, h, one.ctypes.data_as(C.c_void_p))
    np.testing.assert_array_equal(got[0], one)


def test_values_that_land_on_a_byte_boundary(sd, engines):
    """pass-through channels chosen so that m * .5f + .5f is exactly k / 255 or one ulp beside it: the truncation's decision points"""
    e = engines("SD15_TINY")
    k = (np.arange(256, dtype=F) / F(255.0)).astype(F)
    target = np.concatenate([k, np.nextafter(k, F(2)), np.nextafter(k, F(-1))]).astype(F)
    x = np.zeros((1, 3, 8, 96), dtype=F)
    x.reshape(3, -1)[:, :] = ((target - F(0.5)) * F(2.0)).astype(F)[None, :]
    np.testing.assert_array_equal(e.latent_preview(x), ref.latent_preview(x, None, None))


@pytest.mark.parametrize("name", ["SD15_TINY", "SDXL_TINY", "SD35_TINY", "FLUX_TINY", "RGB"])
def test_family_tables_against_the_reference_bytes(sd, engines, name):
    """the fixture's bytes came out of the reference's preview_latent_video (src/runtime/latent-preview.h) run on the fixture's inputs"""
    g = np.load(GOLDEN)
    x, want = g[name + "_latent"][None], g[name + "_bytes"][None]
    e = engines("SD15_TINY" if name == "RGB" else name)
    np.testing.assert_array_equal(e.latent_preview(x), want)
    tab = (None, None) if name == "RGB" else ref.FAMILY_TABLES[name]
    np.testing.assert_array_equal(ref.latent_preview(x, *tab), want)


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("method", ["EULER_A", "HEUN"])
def test_host_loop_callback_sequence(sd, engines, method, interval, noisy):
    e = engines("SD15_TINY")
    rec = Recorder(e)
    try:
        e.set_preview(rec, mode=sd.PREVIEW_PROJ, interval=interval, denoised=True, noisy=noisy)
        sample(sd, e, "SD15_TINY", method=getattr(sd, method))
    finally:
        e.set_preview(None)
    steps = HEUN_STEPS if method == "HEUN" else list(range(1, STEPS + 1))
    assert rec.sequence() == ref.expected_calls(steps, interval, denoised=True, noisy=noisy)
    if method == "HEUN" and interval == 1:
        assert any(s < 0 for s, _ in rec.sequence())
    for c in rec.calls:
        assert c["frames"].shape == (1, 8, 8, 3) and c["first"] == 0 and c["in_scale"] == 1.0
        np.testing.assert_array_equal(c["frames"], ref.latent_preview(c["latent"].reshape(1, 4, 8, 8), *ref.FAMILY_TABLES["SD15_TINY"]))


def test_device_groups_report_their_first_image(sd, engines):
    e = engines("SD15_TINY")
    rec = Recorder()
    try:
        e.set_preview(rec, interval=3)
        sample(sd, e, "SD15_TINY", batch=3, device_batch=2)
    finally:
        e.set_preview(None)
    assert [(c["step"], c["first"], c["frames"].shape[0]) for c in rec.calls] == [(3, 0, 2), (6, 0, 2), (3, 2, 1), (6, 2, 1)]


@pytest.mark.parametrize("device_sampler", [False, True])
@pytest.mark.parametrize("mode", ["PROJ", "TAE", "VAE"])
def test_latents_unchanged_by_a_preview(sd, engines, mode, device_sampler):
    e = engines("SD15_TINY")
    plain = sample(sd, e, "SD15_TINY", device_sampler=device_sampler)
    rec = Recorder(e)
    try:
        e.set_preview(rec, mode=getattr(sd, "PREVIEW_" + mode), interval=3, denoised=True, noisy=True)
        got = sample(sd, e, "SD15_TINY", device_sampler=device_sampler)
    finally:
        e.set_preview(None)
    assert got.tobytes() == plain.tobytes()
    assert rec.sequence() == [(3, True), (3, False), (6, True), (6, False)]
    for c in rec.calls:
        lat = (c["latent"] * F(c["in_scale"])).astype(F).reshape(1, 4, 8, 8) if c["in_scale"] != 1.0 else c["latent"].reshape(1, 4, 8, 8)
        if mode == "PROJ":
            want = ref.latent_preview(c["latent"].reshape(1, 4, 8, 8), *ref.FAMILY_TABLES["SD15_TINY"], in_scale=c["in_scale"])
        elif mode == "TAE":
            want = ref.planar_to_u8(e.tae_decode(lat))
        else:
            want = ref.planar_to_u8(e.vae_decode(lat))
        assert c["frames"].shape == want.shape
        np.testing.assert_array_equal(c["frames"], want)
    # fn = None after a run: no callback fires and the trajectory issues what the plain one did
    n = len(rec.calls)
    again = sample(sd, e, "SD15_TINY", device_sampler=device_sampler)
    assert len(rec.calls) == n and again.tobytes() == plain.tobytes()


def test_spectrum_forecast_calls_deliver_denoised_frames_only(sd, engines):
    e = engines("SD15_TINY")
    steps = 16
    rec = Recorder()
    try:
        e.set_step_cache(sd.CACHE_SPECTRUM)
        e.set_preview(rec, interval=1, denoised=True, noisy=True)
        for device_sampler in (False, True):
            rec.calls.clear()
            sample(sd, e, "SD15_TINY", steps=steps, method=sd.EULER, device_sampler=device_sampler)
            schedule = sd.spectrum_schedule(steps)
            forecast = {i for i, ch in enumerate(schedule) if ch == "P"}
            assert len(forecast) == 6
            assert rec.sequence() == ref.expected_calls(list(range(1, steps + 1)), 1, denoised=True, noisy=True, forecast=forecast)
    finally:
        e.set_preview(None)
        e.set_step_cache(None)


def test_refusals(sd, engines):
    e = engines("SD15_TINY")
    L = sd.lib()
    x = np.zeros((1, 4, 8, 8), dtype=F)
    out = np.zeros((1, 8, 8, 3), dtype=np.uint8)
    e.latent_preview(x)  # (declares the argument types)
    e.planar_to_u8(np.zeros((1, 3, 8, 8), dtype=F))
    assert not L.sdm_latent_preview(e._ctx, None, 8, 8, 4, 1, 1.0, out.ctypes.data_as(C.c_void_p))
    assert not L.sdm_latent_preview(e._ctx, x.ctypes.data_as(C.c_void_p), 8, 8, 4, 1, 1.0, None)
    assert not L.sdm_planar_to_u8(e._ctx, None, 8, 8, 1, out.ctypes.data_as(C.c_void_p))
    big = np.zeros((1, 129, 2, 2), dtype=F)
    with pytest.raises(sd.EngineError):
        e.latent_preview(big)
    with pytest.raises(sd.EngineError):
        e.set_preview_projection(np.zeros((129, 3), dtype=F))
    with pytest.raises(sd.EngineError):
        e.latent_preview(np.zeros((1, 7, 2, 2), dtype=F))  # no table for 7 channels
    # together with a CFG-pair exchange the device sampler refuses an installed preview at sampling time
    try:
        e.set_pair_exchange(lambda ptr, count, stream: True, branch=0)
        e.set_preview(Recorder())
        with pytest.raises(sd.EngineError, match="preview"):
            sample(sd, e, "SD15_TINY", device_sampler=True)
    finally:
        e.set_preview(None)
        e.set_pair_exchange(None)


def test_off_restores_the_plain_run(sd, engines):
    e = engines("SD15_TINY")
    c0 = e.stats()["unet_calls"]
    plain = sample(sd, e, "SD15_TINY")
    plain_calls = e.stats()["unet_calls"] - c0
    rec = Recorder()
    e.set_preview(rec)
    sample(sd, e, "SD15_TINY")
    assert len(rec.calls) == STEPS
    e.set_preview(None)
    c1 = e.stats()["unet_calls"]
    again = sample(sd, e, "SD15_TINY")
    assert len(rec.calls) == STEPS and again.tobytes() == plain.tobytes()
    assert e.stats()["unet_calls"] - c1 == plain_calls
