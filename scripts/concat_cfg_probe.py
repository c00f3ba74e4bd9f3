#!/usr/bin/env python
"""What the c_concat input and the third guidance branch cost on the device-resident sampler, and what the two fused glue launches (k_model_input,
k_guidance3: backend options fuse_model_input / fuse_guidance3) save, in ONE process on one GPU: SD1.5 INPAINT 512x512, batch 8, 20 steps, Euler-A.

  plain pair            a plain SD1.5 context, cond / uncond: the leg to hold against bench.py's line of the same workload
  inpaint, 2 branches   cond / uncond with the 5-channel concat, fusions on and off
  inpaint, 3 branches   + img_uncond (img_cfg 1.5), fusions on and off

The legs alternate over the repetitions (other people's work shares the host: a drift hits every leg alike); every leg's first call builds its plans and is not
timed.  Reports the median last_sample_ms per leg, per step, and whether on / off latents are bit-identical.  Appends to profiles/concat_cfg_probe.txt.

usage: concat_cfg_probe.py [steps=20] [batch=8] [reps=5] [out=FILE]   (synthetic weights: the timing of a step does not depend on them)"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import sdcpp_amd as sd


def main():
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    steps, batch, reps = int(opts.get("steps", 20)), int(opts.get("batch", 8)), int(opts.get("reps", 5))
    path = Path(opts.get("out", ROOT / "profiles" / "concat_cfg_probe.txt"))
    path.parent.mkdir(parents=True, exist_ok=True)
    out = open(path, "a")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    sd.load_mi355x_backend()
    rng = np.random.default_rng(0)
    t0 = time.time()
    plain = sd.Engine(model=sd.SD15, wtype=sd.F16, flash_attn=True)
    inp = sd.Engine(model=sd.SD15, wtype=sd.F16, flash_attn=True, variant=sd.UNET_INPAINT)
    cond, uncond = rng.standard_normal((1, 77, 768)).astype(np.float32), rng.standard_normal((1, 77, 768)).astype(np.float32)
    cat = rng.standard_normal((1, 5, 64, 64)).astype(np.float32)
    cat[:, 0] = cat[:, 0] > 0
    inp.set_concat_condition(cat)
    kw = dict(width=512, height=512, steps=steps, cfg=7.0, seed=42, batch=batch, device_batch=batch, fuse_cfg=True, device_sampler=True, method=sd.EULER_A)
    say(f"== SD1.5 512x512 batch {batch}, {steps} steps, Euler-A, device-resident sampler (contexts made in {time.time() - t0:.0f} s)")

    def leg(engine, img_cfg, fused):
        def run():
            for key in ("fuse_model_input", "fuse_guidance3"):
                sd.backend_set_option(key, fused)
            engine.set_img_cfg(img_cfg)
            lat = engine.sample_latents(cond, uncond, **kw)
            return lat, engine.stats()["last_sample_ms"]
        return run

    legs = [("plain pair", leg(plain, float("inf"), 1)),
            ("inpaint, 2 branches, fused", leg(inp, float("inf"), 1)), ("inpaint, 2 branches, plain nodes", leg(inp, float("inf"), 0)),
            ("inpaint, 3 branches, fused", leg(inp, 1.5, 1)), ("inpaint, 3 branches, plain nodes", leg(inp, 1.5, 0))]
    times = {name: [] for name, _ in legs}
    lats = {}
    for rep in range(reps + 1):   # (an option change drops the cached plans: every timed call is the second of two)
        for name, run in legs:
            run()
            lats[name], ms = run()
            if rep > 0:
                times[name].append(ms)
    for name, _ in legs:
        t = np.array(times[name])
        say(f"   {name:<34} {np.median(t):9.2f} ms   ({np.median(t) / steps:.3f} ms per step; min {t.min():.2f}, max {t.max():.2f} over {t.size} runs)")
    for k in ("2", "3"):
        same = np.array_equal(lats[f"inpaint, {k} branches, fused"], lats[f"inpaint, {k} branches, plain nodes"])
        say(f"   {k} branches: fused vs plain nodes latents {'bit-identical' if same else 'DIFFERENT'}")
    for key in ("fuse_model_input", "fuse_guidance3"):
        sd.backend_set_option(key, 1)
    plain.close()
    inp.close()


if __name__ == "__main__":
    main()
