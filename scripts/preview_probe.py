#!/usr/bin/env python
"""What latent previews (sdm_set_preview_callback) cost on the device-resident sampler, in ONE process on one GPU: SD1.5 512x512, batch 8, 20 steps,

  off              no callback installed: the trajectory as it is without previews (the leg to hold against bench.py's line of the same workload)
  proj, every 1    the projection kernel, a 98 KB copy of the bytes and ONE stream synchronisation after every step
  proj, every 5    the same on steps 5, 10, 15, 20
  tae, every 5     the latent read back (512 KB), the TAESD graph, the byte kernel on its output, 6 MB of bytes, on the same four steps

Reports last_sample_ms (median of the repetitions after the first call, which builds the plans) and the callback count.  Appends to profiles/preview_probe.txt.

usage: preview_probe.py [steps=20] [batch=8] [reps=3] [out=FILE]   (synthetic weights: the timing of a step does not depend on them)"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import sdcpp_amd as sd


def main():
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    steps, batch, reps = int(opts.get("steps", 20)), int(opts.get("batch", 8)), int(opts.get("reps", 3))
    path = Path(opts.get("out", ROOT / "profiles" / "preview_probe.txt"))
    path.parent.mkdir(parents=True, exist_ok=True)
    out = open(path, "a")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    sd.load_mi355x_backend()
    rng = np.random.default_rng(0)
    t0 = time.time()
    e = sd.Engine(model=sd.SD15, wtype=sd.F16, flash_attn=True)
    cond, uncond = rng.standard_normal((1, 77, 768)).astype(np.float32), rng.standard_normal((1, 77, 768)).astype(np.float32)
    kw = dict(width=512, height=512, steps=steps, cfg=7.0, seed=42, batch=batch, device_batch=batch, fuse_cfg=True, device_sampler=True)
    say(f"== SD1.5 512x512 batch {batch}, {steps} steps, device-resident sampler (context made in {time.time() - t0:.0f} s); HIP passes: {e.preview_device_passes()}")
    seen = []

    def run():
        lat, times = None, []
        for _ in range(reps + 1):  # the first call builds the plans
            del seen[:]
            lat = e.sample_latents(cond, uncond, **kw)
            times.append(e.stats()["last_sample_ms"])
        return lat, float(np.median(times[1:])), len(seen)

    e.set_preview(None)
    lat_off, ms_off, _ = run()
    say(f"   off             {ms_off:9.2f} ms   ({ms_off / steps:.2f} ms per step, {ms_off / 1e3 / batch:.4f} s / image)")
    for label, mode, interval in (("proj, every 1", sd.PREVIEW_PROJ, 1), ("proj, every 5", sd.PREVIEW_PROJ, 5), ("tae, every 5", sd.PREVIEW_TAE, 5)):
        e.set_preview(lambda step, frames, noisy, first: seen.append((step, frames.shape)), mode=mode, interval=interval)
        lat, ms, n = run()
        say(f"   {label:<15} {ms:9.2f} ms   (+{ms - ms_off:.2f} ms over the trajectory, {(ms - ms_off) / max(n, 1):.3f} ms per preview; {n} callbacks, frames {seen[-1][1]}; "
            f"latents {'bit-identical' if np.array_equal(lat, lat_off) else 'DIFFERENT'})")
    e.set_preview(None)
    _, ms_again, _ = run()
    say(f"   off again       {ms_again:9.2f} ms")
    e.close()


if __name__ == "__main__":
    main()
