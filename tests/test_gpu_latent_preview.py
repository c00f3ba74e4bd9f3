"""Latent previews on the MI355X backend: the two byte-stage kernels (kernels/preview.hip) against the numpy rules byte for byte, device-resident trajectories
with PROJ previews against the same trajectories without (latents) and against the host loop on the same backend (frames), with UCache / Spectrum armed, and the
TAE / VAE modes against the decoders' own entry points.  With SDCPP_GPU_TESTS_ON_ORACLE=1 both sides run the CPU oracle and the passes are the host restatement.

Every frame of the device sampler is compared with the restatement applied to the tensor the kernel read (Engine.preview_latent inside the callback).  Where the
device sampler and the host loop are bit-identical on this backend (the test establishes it from their final latents and prints it), every frame is also compared
with the restatement applied to the HOST LOOP's `denoised` / `noised` of the same step, captured inside the host loop's callback.  On the MI355X all six pairs
below (SD15_TINY, SD35_TINY, FLUX_TINY x Euler, Euler-A; fuse_cfg, 64 x 64, 6 steps) are bit-identical, so both comparisons run for every frame."""
import os

import numpy as np
import pytest

import latent_preview_ref as ref
from latent_preview_ref import STEPS, Recorder, sample

pytestmark = pytest.mark.gpu
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"
F = np.float32
SHAPES = [(5, 3, 4, 1), (8, 8, 16, 3), (33, 17, 16, 2), (64, 64, 4, 2), (128, 128, 16, 1), (8, 8, 3, 2), (8, 8, 128, 1)]


@pytest.fixture(scope="module")
def engines(sd, gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = sd.Engine(model=getattr(sd, name), backend=gpu, flash_attn=True)
        return made[name]

    return get


def custom_table(c, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((c, 3)) * (0.6 / np.sqrt(c))).astype(F), (rng.standard_normal(3) * 0.05).astype(F)


@pytest.mark.parametrize("shape", SHAPES)
def test_latent_preview_kernel(sd, engines, shape):
    """(5, 3, 4, 1): the scalar path alone; (8, 8, 16, 3): quads, several images; (33, 17, 16, 2): an odd plane (561 floats: the second image's base is not 16-byte
    aligned) takes the scalar path with byte stores throughout; (64, 64, 4, 2): the SD1.5 latent; (128, 128, 16, 1): 4096 quads, more than one workgroup;
    (8, 8, 3, 2): no table; (8, 8, 128, 1): the table's capacity.  About a third of the pixels clamp at each end; zeros, -0.0, NaN and +-inf are in the input."""
    w, h, c, n = shape
    e = engines("SD15_TINY")
    assert e.preview_device_passes() == ON_GPU, "on the MI355X backend the passes are its HIP kernels, never the host restatement"
    proj, bias = (None, None) if c == 3 else custom_table(c, c)
    try:
        e.set_preview_projection(proj, bias)
        x = ref.make_latent((n, c, h, w), 7 * w + c, proj)
        for in_scale in (1.0, 0.4371):
            got = e.latent_preview(x, in_scale)
            np.testing.assert_array_equal(got, ref.latent_preview(x, proj, bias, in_scale))
            assert e.latent_preview(x, in_scale).tobytes() == got.tobytes()
    finally:
        e.set_preview_projection(None)


@pytest.mark.parametrize("name", ["SD15_TINY", "SD35_TINY", "FLUX_TINY"])
def test_family_tables_on_the_device(sd, engines, name):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "latent_preview.npz"))
    np.testing.assert_array_equal(engines(name).latent_preview(g[name + "_latent"][None]), g[name + "_bytes"][None])


@pytest.mark.parametrize("shape", [(5, 3, 1), (64, 64, 2), (67, 31, 3)])
def test_planar_to_u8_kernel(sd, engines, shape):
    """(5, 3): scalar path; (64, 64) x 2: quads; (67, 31) x 3: an odd plane.  Values <= 0, >= 1, k / 255 and (k + 0.5) / 255 with their f32 neighbours."""
    w, h, n = shape
    e = engines("SD15_TINY")
    x = ref.make_image((n, 3, h, w), w)
    got = e.planar_to_u8(x)
    np.testing.assert_array_equal(got, ref.planar_to_u8(x))
    assert e.planar_to_u8(x).tobytes() == got.tobytes()


def frames_of(rec, noisy=False):
    return {c["step"]: c for c in rec.calls if c["noisy"] == noisy}


@pytest.mark.parametrize("method", ["EULER", "EULER_A"])
@pytest.mark.parametrize("name", ["SD15_TINY", "SD35_TINY", "FLUX_TINY"])
def test_device_sampler_trajectory(sd, engines, name, method):
    e = engines(name)
    ch = ref.MODELS[name][2]
    table = ref.FAMILY_TABLES[name]
    over = dict(method=getattr(sd, method))
    plain = sample(sd, e, name, device_sampler=True, **over)
    host_rec = Recorder(e)
    try:
        # the host loop on the same backend: its denoised / noised tensors, captured inside the callback
        e.set_preview(host_rec, interval=1, denoised=True, noisy=True)
        host = sample(sd, e, name, **over)
        bitwise = host.tobytes() == plain.tobytes()
        print(f"{name} {method}: device sampler and host loop bit-identical: {bitwise} (max |diff| {float(np.abs(host - plain).max()):.3e})")
        for interval in (1, 3):
            rec = Recorder(e)
            e.set_preview(rec, interval=interval, denoised=True, noisy=True)
            got = sample(sd, e, name, device_sampler=True, **over)
            # (a) the capture changes no rounding point
            assert got.tobytes() == plain.tobytes()
            assert rec.sequence() == ref.expected_calls(list(range(1, STEPS + 1)), interval, denoised=True, noisy=True)
            # (b) every denoised frame is the restatement of the host loop's denoised of that step
            hd, hn = frames_of(host_rec), frames_of(host_rec, noisy=True)
            for c in rec.calls:
                assert c["frames"].shape == (1, 8, 8, 3) and (c["in_scale"] == 1.0 or c["noisy"])
                np.testing.assert_array_equal(c["frames"], ref.latent_preview(c["latent"].reshape(1, ch, 8, 8), *table, in_scale=c["in_scale"]))
                if bitwise:
                    src = (hn if c["noisy"] else hd)[c["step"]]
                    np.testing.assert_array_equal(c["frames"], ref.latent_preview(src["latent"].reshape(1, ch, 8, 8), *table))
            # (c) the noisy frame of step 1 is the restatement of x0 * c_in: x0 is the same Philox draw on both paths, so the host loop's `noised` of its first
            # call is that tensor whether or not the later steps agree bit for bit
            if interval == 1:
                first = [c for c in rec.calls if c["noisy"] and c["step"] == 1]
                assert len(first) == 1
                np.testing.assert_array_equal(first[0]["frames"], ref.latent_preview(hn[1]["latent"].reshape(1, ch, 8, 8), *table))
    finally:
        e.set_preview(None)


@pytest.mark.parametrize("name,cache", [("SD15_TINY", "ucache"), ("SD15_TINY", "spectrum"), ("SD35_TINY", "spectrum")])
def test_device_sampler_with_a_step_cache_armed(sd, engines, name, cache):
    """(d) the callback sequence follows the schedule rule — a skipped or forecast call still delivers its denoised frame, a forecast call no noisy one — and the
    latents are those of the armed run without a preview"""
    e = engines(name)
    steps = 16
    try:
        if cache == "spectrum":
            e.set_step_cache(sd.CACHE_SPECTRUM)
        else:
            e.set_step_cache(sd.CACHE_UCACHE, reuse_threshold=1.0)
        plain = sample(sd, e, name, steps=steps, method=sd.EULER, device_sampler=True)
        trace = e.step_cache_trace()
        skipped = {i for i, r in enumerate(trace) if r["skipped"]}
        assert len(skipped) == 6 if cache == "spectrum" else len(skipped) > 0  # the skip-step / predicted-step graphs run, with and without the capture
        for interval in (1, 3):
            rec = Recorder()
            e.set_preview(rec, interval=interval, denoised=True, noisy=True)
            got = sample(sd, e, name, steps=steps, method=sd.EULER, device_sampler=True)
            assert got.tobytes() == plain.tobytes()
            assert {i for i, r in enumerate(e.step_cache_trace()) if r["skipped"]} == skipped
            forecast = skipped if cache == "spectrum" else ()
            assert rec.sequence() == ref.expected_calls(list(range(1, steps + 1)), interval, denoised=True, noisy=True, forecast=forecast)
    finally:
        e.set_preview(None)
        e.set_step_cache(None)


@pytest.mark.parametrize("mode", ["TAE", "VAE"])
def test_decode_modes_on_the_device_sampler(sd, engines, mode):
    """interval 3 (TAE: steps 3 and 6) / interval 6 (VAE: one frame): frames [1, 64, 64, 3], byte-equal to the byte rule applied to the decoder's own entry point
    on the latent captured in the callback, computed after the run; the final latents are those of the run without a preview"""
    e = engines("SD15_TINY")
    plain = sample(sd, e, "SD15_TINY", device_sampler=True)
    rec = Recorder(e)
    try:
        e.set_preview(rec, mode=getattr(sd, "PREVIEW_" + mode), interval=3 if mode == "TAE" else 6)
        got = sample(sd, e, "SD15_TINY", device_sampler=True)
    finally:
        e.set_preview(None)
    assert got.tobytes() == plain.tobytes()
    assert rec.sequence() == ([(3, False), (6, False)] if mode == "TAE" else [(6, False)])
    for c in rec.calls:
        assert c["frames"].shape == (1, 64, 64, 3) and c["in_scale"] == 1.0
        lat = c["latent"].reshape(1, 4, 8, 8)
        want = ref.planar_to_u8(e.tae_decode(lat) if mode == "TAE" else e.vae_decode(lat))
        np.testing.assert_array_equal(c["frames"], want)


def test_no_callback_no_trace_of_previews(sd, engines):
    """with previews off after a run with them, a device-sampler trajectory builds no plan and launches what it launched before previews were ever installed"""
    e = engines("SD15_TINY")
    sample(sd, e, "SD15_TINY", device_sampler=True)
    s0 = sd.backend_stats() if ON_GPU else None
    plain = sample(sd, e, "SD15_TINY", device_sampler=True)
    s1 = sd.backend_stats() if ON_GPU else None
    rec = Recorder()
    e.set_preview(rec, interval=3)
    sample(sd, e, "SD15_TINY", device_sampler=True)
    e.set_preview(None)
    s2 = sd.backend_stats() if ON_GPU else None
    again = sample(sd, e, "SD15_TINY", device_sampler=True)
    assert again.tobytes() == plain.tobytes() and len(rec.calls) == 2
    if ON_GPU:
        s3 = sd.backend_stats()
        for k in ("graphs_computed", "plans_built", "kernels_launched"):
            assert s3[k] - s2[k] == s1[k] - s0[k], k
        assert s3["plans_built"] == s2["plans_built"]
