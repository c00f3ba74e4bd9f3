"""NumPy restatements for the inpaint / pix2pix UNet tests (tests/test_concat_cfg_cpu.py, tests/test_gpu_concat_cfg.py): the reference's three-conditioning
guidance combine and its branch rule, the two mask stages of the inpaint condition, and the model input the device-resident sampler assembles.  Every array is
float32 and every operation is one NumPy ufunc call, so each result is rounded to f32 on its own like sd::Tensor<float>'s operators."""
import numpy as np

F = np.float32


def branch_rule(txt_cfg: float, img_cfg: float):
    """resolve_guidance (src/stable-diffusion.cpp:4249-4255): (uncond runs, img_uncond runs)"""
    return (img_cfg != txt_cfg, img_cfg != 1.0)


def cfg_combine3(cond, uncond, img_uncond, txt_cfg, img_cfg):
    """ClassifierFreeGuidance::forward (src/runtime/guidance.cpp:162-176), left to right; uncond / img_uncond None: the two-prediction forms"""
    c = np.asarray(cond, F)
    t, i = F(txt_cfg), F(img_cfg)
    if uncond is not None and img_uncond is not None:
        u, iu = np.asarray(uncond, F), np.asarray(img_uncond, F)
        return (iu + i * (u - iu)) + t * (c - u)
    if uncond is not None:
        u = np.asarray(uncond, F)
        return u + t * (c - u)
    if img_uncond is not None:
        iu = np.asarray(img_uncond, F)
        return iu + t * (c - iu)
    return c.copy()


def _fma(a, b, c):
    """a * b + c rounded once (the product of two f32 is exact in f64)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def cfg_combine3_contracted(cond, uncond, img_uncond, txt_cfg, img_cfg):
    """what a compiler that contracts multiply-adds would compute: fma(txt, c - u, fma(img, u - iu, iu))"""
    c, u, iu = np.asarray(cond, F), np.asarray(uncond, F), np.asarray(img_uncond, F)
    return _fma(F(txt_cfg), c - u, _fma(F(img_cfg), u - iu, iu))


def special_vectors(n: int, seed: int):
    """random f32 vectors seeded with the values that show a careless combine: signed zeros, subnormals, 1e30-scale magnitudes"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        v = (rng.standard_normal(n) * 3).astype(F)
        sp = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, 1e30, -1e30, 2.5e30, 1.17549435e-38], F)
        pos = rng.permutation(n)[: min(n, 3 * sp.size)]
        v[pos] = np.resize(sp, pos.size)[rng.permutation(pos.size)]
        out.append(v)
    return out


def same_bits(a, b) -> bool:
    """bit equality; NaNs (none are expected) only have to sit in the same places"""
    a, b = np.asarray(a, F).ravel(), np.asarray(b, F).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def latent_mask(mask):
    """sd::ops::round (src/core/tensor.hpp:1089-1092: std::round, halves away from zero) then interpolate NearestMax to 1/8 (:1346-1360): the max of every 8x8 block"""
    m = np.asarray(mask, np.float64)
    r = (np.sign(m) * np.floor(np.abs(m) + 0.5)).astype(F)
    h, w = r.shape
    return r.reshape(h // 8, 8, w // 8, 8).max(axis=(1, 3))


def max_pool3(m):
    """sd::ops::max_pool_2d 3x3, stride 1, pad 1 (src/core/tensor.hpp:1473-1544): cells outside the map do not take part"""
    a = np.asarray(m, F)
    p = np.pad(a, 1, constant_values=-np.inf)
    h, w = a.shape
    return np.max([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0).astype(F)


def model_input(x, c_in, concat, k, per_image):
    """x [nb,C,H,W], concat [k or k*nb, cc, H, W] -> [k*nb, C+cc, H, W]: image b*k + j = (x[b] * c_in | concat row j, or row b*k + j when per image)"""
    x, cat = np.asarray(x, F), np.asarray(concat, F)
    nb = x.shape[0]
    scaled = x * F(c_in)
    rows = []
    for b in range(nb):
        for j in range(k):
            rows.append(np.concatenate([scaled[b], cat[b * k + j if per_image else j]], axis=0))
    return np.stack(rows)
