"""Numpy restatement of the latent previews' two byte rules and of the schedule rule (csrc/host/preview.hpp, kernels/preview.hip).  Every operation is rounded
to f32 on its own (numpy float32 arithmetic never contracts) and channels are taken in ascending order, like the reference's preview_latent_video
(src/runtime/latent-preview.h:401-459) and preprocessing_float_to_u8 (src/runtime/preprocessing.hpp:27-35)."""
import numpy as np

F = np.float32
NONE, PROJ, TAE, VAE = 0, 1, 2, 3

# the four families' published latent -> RGB tables (ComfyUI's latent formats; SD3: Stability's sd3_impls.py), as csrc/host/preview.hpp holds them
SD_PROJ = np.array([[0.337366, 0.216344, 0.257386], [0.165636, 0.386828, 0.046994], [-0.267803, 0.237036, 0.223517], [-0.178022, -0.200862, -0.678514]], dtype=F)
SD_BIAS = np.array([-0.017478, -0.055834, -0.105825], dtype=F)
SDXL_PROJ = np.array([[0.258303, 0.277640, 0.329699], [-0.299701, 0.105446, 0.014194], [0.050522, 0.186163, -0.143257], [-0.211938, -0.149892, -0.080036]], dtype=F)
SDXL_BIAS = np.array([0.144381, -0.033313, 0.007061], dtype=F)
SD3_PROJ = np.array([[-0.0645, 0.0177, 0.1052], [0.0028, 0.0312, 0.0650], [0.1848, 0.0762, 0.0360], [0.0944, 0.0360, 0.0889], [0.0897, 0.0506, -0.0364],
                     [-0.0020, 0.1203, 0.0284], [0.0855, 0.0118, 0.0283], [-0.0539, 0.0658, 0.1047], [-0.0057, 0.0116, 0.0700], [-0.0412, 0.0281, -0.0039],
                     [0.1106, 0.1171, 0.1220], [-0.0248, 0.0682, -0.0481], [0.0815, 0.0846, 0.1207], [-0.0120, -0.0055, -0.0867], [-0.0749, -0.0634, -0.0456],
                     [-0.1418, -0.1457, -0.1259]], dtype=F)
SD3_BIAS = np.zeros(3, dtype=F)
FLUX_PROJ = np.array([[-0.041168, 0.019917, 0.097253], [0.028096, 0.026730, 0.129576], [0.065618, -0.067950, -0.014651], [-0.012998, -0.014762, 0.081251],
                      [0.078567, 0.059296, -0.024687], [-0.015987, -0.003697, 0.005012], [0.033605, 0.138999, 0.068517], [-0.024450, -0.063567, -0.030101],
                      [-0.040194, -0.016710, 0.127185], [0.112681, 0.088764, -0.041940], [-0.023498, 0.093664, 0.025543], [0.082899, 0.048320, 0.007491],
                      [0.075712, 0.074139, 0.081965], [-0.143501, 0.018263, -0.136138], [-0.025767, -0.082035, -0.040023], [-0.111849, -0.055589, -0.032361]], dtype=F)
FLUX_BIAS = np.array([0.024600, -0.006937, -0.008089], dtype=F)
FAMILY_TABLES = {"SD15_TINY": (SD_PROJ, SD_BIAS), "SDXL_TINY": (SDXL_PROJ, SDXL_BIAS), "SD35_TINY": (SD3_PROJ, SD3_BIAS), "FLUX_TINY": (FLUX_PROJ, FLUX_BIAS)}


def latent_preview(lat, proj, bias, in_scale=1.0):
    """lat [N, C, h, w] f32 -> uint8 [N, h, w, 3].  proj [C, 3] or None (C == 3: the channels are r, g, b, nothing is added); bias [3] or None (zeros)."""
    lat = np.ascontiguousarray(lat, dtype=F)
    n, c, h, w = lat.shape
    with np.errstate(all="ignore"):
        v = lat if F(in_scale) == F(1.0) else lat * F(in_scale)  # one rounded multiply, only when in_scale != 1
        if proj is None:
            assert c == 3
            acc = [v[:, k] for k in range(3)]
        else:
            proj = np.asarray(proj, dtype=F)
            assert proj.shape == (c, 3)
            b = np.zeros(3, dtype=F) if bias is None else np.asarray(bias, dtype=F)
            acc = []
            for k in range(3):
                a = np.zeros((n, h, w), dtype=F)
                for d in range(c):
                    a = a + v[:, d] * proj[d, k]  # the product rounds, then the sum
                acc.append(a + b[k])
        out = np.empty((n, h, w, 3), dtype=np.uint8)
        for k in range(3):
            m = acc[k] * F(0.5) + F(0.5)
            m = np.where(F(0.0) < m, m, F(0.0)).astype(F)  # std::max(0.0f, m): NaN -> 0
            m = np.where(m < F(1.0), m, F(1.0)).astype(F)  # std::min(1.0f, m)
            out[..., k] = (m * F(255.0)).astype(np.int32).astype(np.uint8)  # truncation
    return out


def planar_to_u8(rgb, mul=1.0, add=0.0):
    """rgb [N, 3, H, W] f32 -> uint8 [N, H, W, 3]: v = x * mul + add (only when (mul, add) != (1, 0)); v <= 0 or NaN -> 0, v >= 1 -> 255, else
    (uint8_t)(v * 255.0f + 0.5f)."""
    x = np.ascontiguousarray(rgb, dtype=F)
    with np.errstate(all="ignore"):
        v = x if (F(mul) == F(1.0) and F(add) == F(0.0)) else x * F(mul) + F(add)
        inner = (v > F(0.0)) & (v < F(1.0))
        r = np.where(inner, v, F(0.0)).astype(F) * F(255.0) + F(0.5)
        b = np.where(v >= F(1.0), 255, np.where(inner, r.astype(np.int32), 0)).astype(np.uint8)
    return np.ascontiguousarray(b.transpose(0, 2, 3, 1))


def make_latent(shape, seed, proj=None, specials=True):
    """a latent [N, C, h, w] scaled so that about a third of the projected pixels clamp at each end (the projected value has standard deviation 2.3, it clamps
    beyond +-1), with exact zeros, -0.0, NaN and +-inf placed in it"""
    n, c, h, w = shape
    rng = np.random.default_rng(seed)
    scale = 2.3 if proj is None else 2.3 / max(float(np.sqrt((np.asarray(proj, dtype=np.float64) ** 2).sum(0)).mean()), 1e-6)
    x = (rng.standard_normal(shape) * scale).astype(F)
    flat = x.reshape(n, c, -1)
    flat[:, :, 0] = 0.0
    if specials and h * w >= 8:
        flat[:, :, 4] = -0.0
        flat[0, 0, 1] = np.nan
        flat[0, c - 1, 2] = np.inf
        flat[n - 1, 0, 3] = -np.inf
        flat[n - 1, c - 1, 5] = np.nan
    return x


def make_image(shape, seed):
    """an image [N, 3, H, W] with values <= 0, >= 1, inside (0, 1), and k / 255 and its two f32 neighbours for every k (where a rounding rule shows)"""
    n, _, h, w = shape
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 0.6 + 0.5).astype(F)
    flat = x.reshape(-1)
    k = (np.arange(256, dtype=F) / F(255.0)).astype(F)
    halves = ((np.arange(256, dtype=F) + F(0.5)) / F(255.0)).astype(F)  # where v * 255 + 0.5 crosses an integer
    marks = np.concatenate([k, np.nextafter(k, F(2)), np.nextafter(k, F(-1)), halves, np.nextafter(halves, F(2)), np.nextafter(halves, F(-1)),
                            np.array([0.0, -0.0, 1.0, -3.5, 7.25], dtype=F)]).astype(F)
    m = min(marks.size, flat.size)
    flat[:m] = marks[:m]
    return x


MODELS = {  # name -> (context shape, y width, latent channels)
    "SD15_TINY": ((1, 77, 64), None, 4),
    "SD35_TINY": ((1, 40, 96), 64, 16),
    "FLUX_TINY": ((1, 24, 96), 64, 16),
}
STEPS = 6


def conditioning(name):
    cshape, ydim, _ = MODELS[name]
    rng = np.random.default_rng(5)
    cond, uncond = rng.standard_normal(cshape).astype(F), rng.standard_normal(cshape).astype(F)
    y = None if ydim is None else rng.standard_normal((1, ydim)).astype(F)
    uy = None if ydim is None else rng.standard_normal((1, ydim)).astype(F)
    return cond, uncond, y, uy


def sample(sd, e, name, **over):
    cond, uncond, y, uy = conditioning(name)
    kw = dict(width=64, height=64, steps=STEPS, cfg=4.0, seed=11, batch=1, method=sd.EULER_A, cond_y=y, uncond_y=uy, fuse_cfg=True)
    kw.update(over)
    return e.sample_latents(cond, uncond if kw["cfg"] != 1.0 else None, **kw)


class Recorder:
    """a preview callback that keeps what it is handed: (step, is_noisy, first_image, frames copy[, latent copy, in_scale])"""

    def __init__(self, engine=None):
        self.engine, self.calls = engine, []

    def __call__(self, step, frames, is_noisy, first_image):
        rec = dict(step=step, noisy=is_noisy, first=first_image, frames=frames.copy())
        if self.engine is not None:
            rec["latent"], rec["in_scale"] = self.engine.preview_latent()
        self.calls.append(rec)

    def sequence(self):
        return [(c["step"], c["noisy"]) for c in self.calls]


def due(step, interval):
    """the schedule rule: a denoise call with sampler step s is previewed when |s| % max(interval, 1) == 0"""
    return abs(step) % max(interval, 1) == 0


def expected_calls(steps_of_calls, interval, denoised=True, noisy=False, forecast=()):
    """the (step, is_noisy) sequence a trajectory delivers: per denoise call the noisy frame first (never on a Spectrum-forecast call), then the denoised one.
    steps_of_calls: the step value of every denoise call in order; forecast: indices of the calls Spectrum forecasts."""
    out = []
    for i, s in enumerate(steps_of_calls):
        if not due(s, interval):
            continue
        if noisy and i not in forecast:
            out.append((s, True))
        if denoised:
            out.append((s, False))
    return out
