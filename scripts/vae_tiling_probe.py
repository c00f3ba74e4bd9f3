#!/usr/bin/env python
"""Tiled VAE decode on SD1.5's real VAE (synthetic weights), N = 1, tile 32 / overlap 0.5 (the reference's defaults): wall time of one
vae_decode(raw=True) — crops, uploads, tile graphs, device merge and the read-back of the canvas, ending in a device synchronise — per tile_batch, with
the fused merge on and off at the chosen batch, next to the untiled decode where it exists (128^2 latent), and whether a 512^2 latent completes.

usage: vae_tiling_probe.py [out.txt] [--sizes 128,256] [--big 512] [--repeats 5]
The default tile_batch of the engine is the smallest batch within 3 % of the best median at the 256^2 latent."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import sdcpp_amd as sd

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default="")
ap.add_argument("--sizes", default="128,256")
ap.add_argument("--big", type=int, default=512)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--model", default="SD15")
args = ap.parse_args()

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()   # ends in the read-back of the canvas (synchronises the stream)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


sd.load_mi355x_backend()
cal = sd.calibrate()
say(f"measured_peaks: {cal}")
e = sd.Engine(model=getattr(sd, args.model), backend="MI355X0", flash_attn=True)
ch = 16 if args.model.startswith(("SD35", "FLUX")) else 4
BATCHES = (1, 2, 4, 8, 16)
chosen = None
for lat in [int(v) for v in args.sizes.split(",") if v]:
    z = (np.random.default_rng(lat).standard_normal((1, ch, lat, lat)) * 0.18215 * 2).astype(np.float32)
    tiles = len(sd.tiling_plan(lat, lat)["tiles"])
    say(f"\n== {lat}^2 latent ({lat * 8}^2 pixels), {tiles} tiles of 32 x 32 cells, overlap 0.5; median / min / max of {args.repeats} calls after 2 warm-up calls, ms")
    if lat <= 128:
        # on an engine of its own: a runner's compute buffer only grows, and the tiled rows below report theirs
        e0 = sd.Engine(model=getattr(sd, args.model), backend="MI355X0", flash_attn=True)
        med, lo, hi = timed(lambda: e0.vae_decode(z, raw=True), args.repeats)
        say(f"untiled (for orientation: another computation)   {med:9.1f} {lo:9.1f} {hi:9.1f}")
        e0.close()
    res = {}
    for tb in BATCHES:
        e.set_vae_tiling(True, tile_batch=tb)
        s0 = sd.backend_stats()
        med, lo, hi = timed(lambda: e.vae_decode(z, raw=True), args.repeats)
        s1 = sd.backend_stats()
        res[tb] = med
        say(f"tile_batch {tb:2d}                                     {med:9.1f} {lo:9.1f} {hi:9.1f}   compute buffer {e.stats()['compute_buffer_bytes'] / 2**20:8.0f} MiB"
            f"   graph replays {s1['graph_replays'] - s0['graph_replays']}, plans built {s1['plans_built'] - s0['plans_built']}")
    best = min(res.values())
    pick = min(tb for tb in BATCHES if res[tb] <= best * 1.03)
    say(f"best {best:.1f} ms; smallest batch within 3 %: tile_batch {pick}")
    chosen = pick
    # fused merge off / on at that batch, alternating (the option drops cached plans: each leg warms up again)
    ab = {0: [], 1: []}
    e.set_vae_tiling(True, tile_batch=pick)
    for rep in range(2):
        for on in (0, 1):
            sd.backend_set_option("fuse_tile_merge", on)
            ab[on].append(timed(lambda: e.vae_decode(z, raw=True), args.repeats)[0])
    sd.backend_set_option("fuse_tile_merge", 1)
    say(f"fuse_tile_merge at tile_batch {pick}: off {ab[0][0]:.1f} / {ab[0][1]:.1f} ms, on {ab[1][0]:.1f} / {ab[1][1]:.1f} ms (medians of two alternating legs)")
    # the merge launches alone (family 11: binary elementwise + k_tile_merge), eager with HIP events
    for on in (0, 1):
        sd.backend_set_option("fuse_tile_merge", on)
        e.vae_decode(z, raw=True)
        sd.kernel_timing_enable(1 << 11)
        e.vae_decode(z, raw=True)
        fam = [f for f in sd.kernel_timings() if f["family"] == 11]
        sd.kernel_timing_enable(0)
        if fam:
            say(f"   family 11 with fuse_tile_merge {on}: {fam[0]['launches']} launches, {fam[0]['total_ms']:.3f} ms")
    sd.backend_set_option("fuse_tile_merge", 1)

if args.big:
    lat = args.big
    z = (np.random.default_rng(lat).standard_normal((1, ch, lat, lat)) * 0.18215 * 2).astype(np.float32)
    e.set_vae_tiling(True, tile_batch=chosen or 0)
    say(f"\n== {lat}^2 latent ({lat * 8}^2 pixels), {len(sd.tiling_plan(lat, lat)['tiles'])} tiles, tile_batch {chosen or 'default'}")
    try:
        t0 = time.perf_counter()
        out = e.vae_decode(z, raw=True)
        t1 = time.perf_counter()
        out = e.vae_decode(z, raw=True)
        t2 = time.perf_counter()
        say(f"completed: first call {(t1 - t0) * 1e3:.0f} ms, second {(t2 - t1) * 1e3:.0f} ms, all finite {bool(np.isfinite(out).all())}, "
            f"peak compute buffer {e.stats()['compute_buffer_bytes'] / 2**20:.0f} MiB, canvas {out.nbytes / 2**20:.0f} MiB")
    except sd.EngineError as err:
        say(f"did NOT complete: {err}")

if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
