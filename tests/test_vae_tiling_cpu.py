"""VAE tiling (the reference's `--vae-tiling`) on the CPU oracle backend: the tile plan against known answers and a numpy restatement, the overlap
merge as a partition of unity, the whole tiled decode / encode bit for bit against a driver written here (crop in numpy, one-tile decode through the
same engine, numpy merge: tests/vae_tiling_ref.py), and the context-state behaviour of sd_set_vae_tiling."""
import numpy as np
import pytest

import vae_tiling_ref as ref

# (small, tile, target overlap) -> count, overlap in cells, (start, skip) per tile: from an independent restatement of sd_tiling_calc_tiles + process_tiles_2d
PLAN_KNOWN = [
    ((20, 8, 0.5), 4, 4, [(0, 0), (4, 0), (8, 0), (12, 0)]),
    ((19, 8, 0.3), 3, 2, [(0, 0), (6, 0), (11, 1)]),
    ((17, 8, 0.5), 3, 3, [(0, 0), (5, 0), (9, 1)]),
    ((14, 8, 0.5), 2, 2, [(0, 0), (6, 0)]),
    ((11, 8, 0.25), 2, 5, [(0, 0), (3, 0)]),
    ((9, 4, 0.0), 3, 1, [(0, 0), (3, 0), (5, 1)]),
    ((6, 8, 0.5), 1, 0, [(0, 0)]),
    ((256, 32, 0.5), 15, 16, [(16 * i, 0) for i in range(15)]),
]


@pytest.mark.parametrize("case,count,overlap,pos", PLAN_KNOWN)
def test_plan_known_answers(sd, case, count, overlap, pos):
    small, tile, target = case
    # x axis under test, y axis another case: the axes are independent
    p = sd.tiling_plan(small, 19, tile_size_x=tile, tile_size_y=8, target_overlap=target)
    xs = [(x, dx) for (x, y, dx, dy) in p["tiles"] if y == 0]
    assert len(xs) == count and p["overlap"][0] == overlap and xs == pos
    assert p["tile_size"][0] == min(tile, small)
    # ... and as the y axis: y is the outer loop
    q = sd.tiling_plan(9, small, tile_size_x=4, tile_size_y=tile, target_overlap=target)
    ys = [(y, dy) for (x, y, dx, dy) in q["tiles"] if x == 0]
    assert ys == pos and q["overlap"][1] == overlap
    inner = len(q["tiles"]) // len(ys)
    assert [t[1] for t in q["tiles"]] == [y for (y, _) in pos for _ in range(inner)]


def test_tile_size_rules(sd):
    # rel_size in (0, 1]: a fraction of the latent size, rounded
    assert sd.tiling_plan(40, 30, rel_size_x=0.5, rel_size_y=0.5)["tile_size"] == (20, 15)
    # rel_size > 1: a tile COUNT: size = round(latent / (count - count * overlap + overlap))
    p = sd.tiling_plan(64, 64, rel_size_x=3, rel_size_y=3, target_overlap=0.25)
    assert p["tile_size"] == (26, 26) and len(p["tiles"]) == 9          # 64 / 2.5 = 25.6
    # rel_size wins over tile_size; a request below 4 is the default 32; clamps to [4, latent]
    assert sd.tiling_plan(64, 64, tile_size_x=8, tile_size_y=3, rel_size_x=0.25)["tile_size"] == (16, 32)
    assert sd.tiling_plan(20, 64, tile_size_x=3, tile_size_y=0)["tile_size"] == (20, 32)
    assert sd.tiling_plan(64, 64, rel_size_x=0.01, rel_size_y=0.01)["tile_size"] == (4, 4)
    # the overlap is clamped to [0, 0.5]
    assert sd.tiling_plan(64, 64, tile_size_x=16, tile_size_y=16, target_overlap=0.9) == sd.tiling_plan(64, 64, tile_size_x=16, tile_size_y=16, target_overlap=0.5)
    assert sd.tiling_plan(64, 64, tile_size_x=16, tile_size_y=16, target_overlap=-1.0) == sd.tiling_plan(64, 64, tile_size_x=16, tile_size_y=16, target_overlap=0.0)
    # encode factor 2: the image VAE's encoder takes tiles of twice the size (default 64, one tile for a 512-pixel image)
    assert sd.tiling_plan(64, 64, encode_factor=2.0)["tiles"] == [(0, 0, 0, 0)]
    assert sd.tiling_plan(100, 64, tile_size_x=10, tile_size_y=10, encode_factor=2.0)["tile_size"] == (20, 20)


def test_plan_matches_numpy_restatement(sd):
    rng = np.random.default_rng(11)
    for _ in range(400):
        w, h = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        kw = dict(tile_size_x=int(rng.integers(0, 70)), tile_size_y=int(rng.integers(0, 70)), target_overlap=float(np.float32(rng.uniform(-0.1, 0.7))))
        if rng.random() < 0.3:
            kw["rel_size_x"] = float(np.float32(rng.uniform(0.05, 5.0)))
            kw["rel_size_y"] = float(np.float32(rng.uniform(0.05, 5.0)))
        kw["encode_factor"] = 2.0 if rng.random() < 0.3 else 1.0
        assert sd.tiling_plan(w, h, **kw) == ref.plan(w, h, **kw), (w, h, kw)


@pytest.fixture(scope="module")
def eng15(sd, oracle):
    return sd.Engine(model=sd.SD15_TINY, backend=oracle)


@pytest.fixture(scope="module")
def eng35(sd, oracle):
    return sd.Engine(model=sd.SD35_TINY, backend=oracle)


def ulp_distance_from_one(a):
    return np.abs(a.astype(np.float64) - 1.0) / float(np.spacing(np.float32(1.0)))


@pytest.mark.parametrize("w,h,tx,ty,ov,batch", [
    (20, 19, 8, 8, 0.5, 0), (19, 17, 8, 8, 0.3, 3), (17, 14, 8, 8, 0.5, 1), (14, 20, 8, 8, 0.5, 0), (11, 9, 8, 4, 0.25, 2), (9, 11, 4, 8, 0.0, 0),
    (6, 20, 8, 8, 0.5, 0),    # one tile along x
    (8, 8, 4, 4, 0.0, 3),     # both overlaps 0: the store path
    (64, 40, 32, 32, 0.5, 0),
])
def test_partition_of_unity(sd, eng15, w, h, tx, ty, ov, batch):
    """The ramps of the tiles that cover a cell sum to 1 (a property of the reference's ramps and positions, whoever restates them): tiles of ones blend to ones"""
    eng15.set_vae_tiling(True, tile_size_x=tx, tile_size_y=ty, target_overlap=ov, tile_batch=batch)
    try:
        p = sd.tiling_plan(w, h, tile_size_x=tx, tile_size_y=ty, target_overlap=ov)
        if (w, h) == (8, 8):
            assert p["overlap"] == (0, 0) and len(p["tiles"]) == 4
        out = eng15.tiling_blend(np.ones((2, 3, h, w), np.float32))
        d = ulp_distance_from_one(out)
        print(f"{w}x{h} tile {tx}x{ty} overlap {ov}: {len(p['tiles'])} tiles, overlap cells {p['overlap']}, max |canvas - 1| = {d.max():.2f} ulp")
        assert d.max() <= 4.0
        # the numpy restatement of the merge gives the same bits as the device merge, on a random field too
        x = np.random.default_rng(w * 100 + h).standard_normal((2, 3, h, w)).astype(np.float32)
        np.testing.assert_array_equal(eng15.tiling_blend(x), _blend_ref(x, p))
    finally:
        eng15.set_vae_tiling(False)


def _blend_ref(x, p):
    canvas = np.zeros_like(x)
    tx, ty = p["tile_size"]
    for (px, py, dx, dy) in p["tiles"]:
        ref.merge(canvas, x[:, :, py:py + ty, px:px + tx], px, py, p["overlap"][0], p["overlap"][1], dx, dy)
    return canvas


def one_tile_decode(e, crop):
    """The raw decoder output of one crop through the tiled path itself: a tile size that yields one tile"""
    n, c, h, w = crop.shape
    e.set_vae_tiling(True, tile_size_x=max(w, 4), tile_size_y=max(h, 4), target_overlap=0.0)
    return e.vae_decode(crop, raw=True)


def reference_tiled_decode(sd, e, z, tile, overlap):
    p = sd.tiling_plan(z.shape[3], z.shape[2], tile_size_x=tile, tile_size_y=tile, target_overlap=overlap)
    return ref.tiled(z, lambda crop: one_tile_decode(e, crop), p, decode=True, out_channels=3), p


@pytest.fixture(scope="module")
def decode_cases(sd, eng15, eng35):
    """(engine, latent, numpy-driver result) per case, computed once"""
    rng = np.random.default_rng(5)
    cases = {}
    for name, e, ch, scale in (("sd15", eng15, 4, 0.18215), ("sd35", eng35, 16, 1.5305)):
        for (w, h, n) in ((19, 17, 1), (20, 14, 2)):
            z = (rng.standard_normal((n, ch, h, w)) * scale * 2).astype(np.float32)
            want, p = reference_tiled_decode(sd, e, z, 8, 0.5)
            e.set_vae_tiling(False)
            cases[(name, w, h, n)] = (e, z, want, p)
    return cases


@pytest.mark.parametrize("key", [("sd15", 19, 17, 1), ("sd15", 20, 14, 2), ("sd35", 19, 17, 1), ("sd35", 20, 14, 2)])
def test_tiled_decode_bit_for_bit(decode_cases, key):
    e, z, want, p = decode_cases[key]
    try:
        got = {}
        for tb in (1, 3, 0):
            e.set_vae_tiling(True, tile_size_x=8, tile_size_y=8, target_overlap=0.5, tile_batch=tb)
            got[tb] = e.vae_decode(z, raw=True)
        assert len(p["tiles"]) >= 6 and np.isfinite(want).all()
        np.testing.assert_array_equal(got[1], want)
        np.testing.assert_array_equal(got[3], want)
        np.testing.assert_array_equal(got[0], want)
        # sd_vae_decode = the raw call + (x + 1) / 2 and the clamp, applied once to the merged canvas
        np.testing.assert_array_equal(e.vae_decode(z), np.clip((want + np.float32(1)) * np.float32(0.5), 0, 1))
    finally:
        e.set_vae_tiling(False)


@pytest.mark.parametrize("name", ["sd15", "sd35"])
def test_tiled_encode_bit_for_bit(sd, eng15, eng35, name):
    e = eng15 if name == "sd15" else eng35
    rng = np.random.default_rng(6)
    img = rng.random((1, 3, 152, 136)).astype(np.float32)   # latent 17 x 19: tiles of 4 x factor 2 = 8 cells at odd offsets
    p = sd.tiling_plan(17, 19, tile_size_x=4, tile_size_y=4, target_overlap=0.5, encode_factor=2.0)
    assert p["tile_size"] == (8, 8) and any(t[2] or t[3] for t in p["tiles"])
    zc2 = 2 * (4 if name == "sd15" else 16)

    def one_tile(crop):
        e.set_vae_tiling(True, tile_size_x=4, tile_size_y=4, target_overlap=0.0)
        assert crop.shape[2:] == (64, 64)
        return e.vae_encode(crop, return_moments=True)[1]
    try:
        want = ref.tiled(img, one_tile, p, decode=False, out_channels=zc2)
        got = {}
        for tb in (1, 3, 0):
            e.set_vae_tiling(True, tile_size_x=4, tile_size_y=4, target_overlap=0.5, tile_batch=tb)
            lat, got[tb] = e.vae_encode(img, seed=9, return_moments=True)
        for tb in (1, 3, 0):
            np.testing.assert_array_equal(got[tb], want)
        # the Gaussian sample and the latent scaling run on the MERGED moments
        e.set_vae_tiling(False)
        zc = zc2 // 2
        mean, logvar = want[:, :zc], want[:, zc:]
        noise = sd.philox_randn(9, 0, mean.size).reshape(mean.shape)
        sf, sh = (0.18215, 0.0) if name == "sd15" else (1.5305, 0.0609)
        z = (mean + np.exp(np.float32(0.5) * np.clip(logvar, -30, 20)) * noise - np.float32(sh)) * np.float32(sf)
        np.testing.assert_allclose(lat, z, rtol=1e-5, atol=1e-6)
    finally:
        e.set_vae_tiling(False)


def test_tiling_changes_pixels_and_off_is_exact(sd, oracle, eng15, decode_cases):
    _, z, want, _ = decode_cases[("sd15", 19, 17, 1)]
    never = sd.Engine(model=sd.SD15_TINY, backend=oracle)   # an engine that was never given tiling parameters
    plain = never.vae_decode(z)
    try:
        eng15.set_vae_tiling(True, tile_size_x=8, tile_size_y=8)
        tiled = eng15.vae_decode(z)
        assert not np.array_equal(tiled, plain)   # every tile sees only its own GroupNorm statistics and attention context
        mse = float(np.mean((tiled.astype(np.float64) - plain) ** 2))
        print(f"tiled (8, overlap 0.5) vs untiled decode of a 19 x 17 latent: PSNR {10 * np.log10(1.0 / max(mse, 1e-20)):.1f} dB")
        eng15.set_vae_tiling(False)
        np.testing.assert_array_equal(eng15.vae_decode(z), plain)
        eng15.set_vae_tiling(True, tile_size_x=8, tile_size_y=8)
        eng15.set_vae_tiling(None)                # NULL
        np.testing.assert_array_equal(eng15.vae_decode(z, raw=True), never.vae_decode(z, raw=True))
    finally:
        eng15.set_vae_tiling(False)


def test_generate_image_decodes_tiled(sd, eng15):
    rng = np.random.default_rng(3)
    cond = rng.standard_normal((1, 77, 64)).astype(np.float32)
    kw = dict(width=128, height=64, steps=1, cfg=1.0, seed=5, batch=2)
    try:
        eng15.set_vae_tiling(True, tile_size_x=8, tile_size_y=8, target_overlap=0.5)
        img = eng15.generate_image(cond, None, **kw)
        lat = eng15.sample_latents(cond, None, **kw)
        rgb = eng15.vae_decode(lat)
        np.testing.assert_array_equal(img, np.stack([sd.planar_rgb_to_u8(rgb[i]) for i in range(2)]))
        eng15.set_vae_tiling(False)
        assert not np.array_equal(img, eng15.generate_image(cond, None, **kw))
    finally:
        eng15.set_vae_tiling(False)


def test_canvas_is_cleared_between_calls(eng15, decode_cases):
    _, z, want, _ = decode_cases[("sd15", 19, 17, 1)]
    try:
        eng15.set_vae_tiling(True, tile_size_x=8, tile_size_y=8, target_overlap=0.5)
        other = eng15.vae_decode(z * np.float32(-0.5) + np.float32(0.1), raw=True)   # same shape: the canvas of this call is reused by the next
        np.testing.assert_array_equal(eng15.vae_decode(z, raw=True), want)
        assert not np.array_equal(other, want)
    finally:
        eng15.set_vae_tiling(False)
