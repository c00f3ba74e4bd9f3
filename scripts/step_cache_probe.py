#!/usr/bin/env python
"""What the step caches (sd_set_step_cache) buy and cost on the device-resident sampler, per model family, in ONE process on one GPU:

  off        the trajectory as it is without a cache
  armed, 0   cache armed with reuse_threshold 0: probe pass, 16-byte read-back, recording graph and record pass on every active step, nothing skipped —
             the price of the per-step synchronisation (the build-ahead overlap is gone on active steps)
  default    the reference's default parameters (EasyCache 0.2 / UCache 1.0, window 0.15 .. 0.95): steps skipped, seconds per image, and the PSNR of the decoded
             images against the uncached ones

With modes=new the same workloads run the reference's other four cache modes at its defaults instead — dbcache, taylorseer and cache-dit (one cache under three
names, DiT families only: on a UNet family the line says that they are not armed) and spectrum — each against cache off in the same process: steps skipped,
seconds per image, PSNR of the decoded image against the uncached one.

usage: step_cache_probe.py [sd15] [sdxl] [sd35] [flux] [steps=20] [modes=new] [out=FILE]   (weights are the engine's synthetic ones: the skip counts say what THESE models do,
not what a trained checkpoint does; the timing of a computed, a skipped and an armed step does not depend on the weights)"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import sdcpp_amd as sd

FAMILIES = {
    # name: (model, wtype, mode, width, batch, context shape, y width, label)
    "sd15": (sd.SD15, sd.F16, sd.CACHE_UCACHE, 512, 8, (1, 77, 768), None, "SD1.5 512x512 batch 8 (UCache)"),
    "sdxl": (sd.SDXL, sd.Q8_0, sd.CACHE_UCACHE, 1024, 1, (1, 77, 2048), 2816, "SDXL 1024x1024 q8_0 (UCache)"),
    "sd35": (sd.SD35_LARGE, sd.BF16, sd.CACHE_EASYCACHE, 1024, 1, (1, 154, 4096), 2048, "SD3.5-large 1024x1024 bf16 (EasyCache)"),
    "flux": (sd.FLUX_DEV, sd.Q4_0, sd.CACHE_EASYCACHE, 1024, 1, (1, 256, 4096), 768, "FLUX.1-dev 1024x1024 q4_0 (EasyCache)"),
}


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b) ** 2))
    return 10 * np.log10(1.0 / max(mse, 1e-20))


def main():
    names = [a for a in sys.argv[1:] if "=" not in a] or list(FAMILIES)
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    steps = int(opts.get("steps", 20))
    out = open(opts["out"], "a") if "out" in opts else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    sd.load_mi355x_backend()
    rng = np.random.default_rng(0)
    for name in names:
        model, wtype, mode, width, batch, cshape, ydim, label = FAMILIES[name]
        t0 = time.time()
        e = sd.Engine(model=model, wtype=wtype, flash_attn=True)
        cond, uncond = rng.standard_normal(cshape).astype(np.float32), rng.standard_normal(cshape).astype(np.float32)
        y = None if ydim is None else rng.standard_normal((1, ydim)).astype(np.float32)
        uy = None if ydim is None else rng.standard_normal((1, ydim)).astype(np.float32)
        flux = name == "flux"  # distilled guidance: one forward per step
        kw = dict(width=width, height=width, steps=steps, cfg=1.0 if flux else 7.0, seed=42, batch=batch, device_batch=batch, cond_y=y, uncond_y=uy, fuse_cfg=True,
                  device_sampler=True)
        say(f"== {label}, {steps} steps, device-resident sampler (context made in {time.time() - t0:.0f} s)")

        def run(reps=2):
            lat, times = None, []
            for _ in range(reps + 1):  # the first call builds the plans
                lat = e.sample_latents(cond, None if flux else uncond, **kw)
                times.append(e.stats()["last_sample_ms"])
            return lat, float(np.median(times[1:])), e.stats()["steps_skipped"], e.step_cache_trace()

        e.set_step_cache(None)
        lat_off, ms_off, _, _ = run()
        if opts.get("modes") == "new":
            img_off = e.vae_decode(lat_off[:1])
            say(f"   off          {ms_off / 1e3 / batch:8.4f} s / image   ({ms_off / steps:.2f} ms per step)")
            for label_, mode_ in (("dbcache", sd.CACHE_DBCACHE), ("taylorseer", sd.CACHE_TAYLORSEER), ("cache-dit", sd.CACHE_CACHE_DIT), ("spectrum", sd.CACHE_SPECTRUM)):
                e.set_step_cache(mode_)
                lat_on, ms_on, skipped, tr_on = run()
                status = e.step_cache_status()
                if status != label_:
                    say(f"   {label_:<12} {status}")
                    continue
                say(f"   {label_:<12} {ms_on / 1e3 / batch:8.4f} s / image   ({skipped} of {steps} steps skipped, {sum(r['active'] for r in tr_on)} active; {ms_off / ms_on:.3f}x; "
                    f"PSNR of the decoded image against the uncached one {psnr(e.vae_decode(lat_on[:1]), img_off):.1f} dB; latents {'finite' if np.isfinite(lat_on).all() else 'NOT FINITE'})")
                say(f"   {'':<12} skipped steps: " + (" ".join(str(r["step"]) for r in tr_on if r["skipped"]) or "none"))
            e.set_step_cache(None)
            e.close()
            continue
        e.set_step_cache(mode, reuse_threshold=0.0)
        lat_zero, ms_zero, _, tr_zero = run()
        e.set_step_cache(mode)
        lat_on, ms_on, skipped, tr_on = run()
        e.set_step_cache(None)
        active = sum(r["active"] for r in tr_on)
        per_step = ms_off / steps
        say(f"   off        {ms_off / 1e3 / batch:8.4f} s / image   ({per_step:.2f} ms per step)")
        say(f"   armed, 0   {ms_zero / 1e3 / batch:8.4f} s / image   (+{ms_zero - ms_off:.2f} ms over the trajectory = {(ms_zero - ms_off) / per_step:.2f} computed steps; "
            f"{sum(r['active'] for r in tr_zero)} active steps; latents {'bit-identical' if np.array_equal(lat_zero, lat_off) else 'DIFFERENT'})")
        say(f"   default    {ms_on / 1e3 / batch:8.4f} s / image   ({skipped} of {steps} steps skipped, {active} active; {ms_off / ms_on:.3f}x)")
        img_off, img_on = e.vae_decode(lat_off[:1]), e.vae_decode(lat_on[:1])
        say(f"   decoded image (first of the batch) against the uncached one: PSNR {psnr(img_on, img_off):.1f} dB")
        say("   skipped steps: " + " ".join(str(r["step"]) for r in tr_on if r["skipped"]))
        e.close()


if __name__ == "__main__":
    main()
