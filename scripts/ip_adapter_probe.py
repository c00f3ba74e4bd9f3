#!/usr/bin/env python
"""What image tokens (IP-Adapter, sd_set_ip_adapter) cost on the device-resident sampler, and what the fused dual-KV attention launch (k_flash_short_ip, backend
option fuse_ip_attn) saves against the plain-node route — two flash launches, SCALE, ADD, with Q written twice as f32 — in ONE process on one GPU, on synthetic
weights, 20 steps of Euler-A with the CFG pair in one graph:

  SD1.5 512x512, batch 8                                             SDXL 1024x1024, batch 1

  adapter off           no tokens set (the graphs of a context without the adapter)
  4 tokens, plain       fuse_ip_attn=0: launches the parent commit has
  4 tokens, fused       fuse_ip_attn=1
  16 tokens, fused

The legs alternate over the repetitions (other people's work shares the host: a drift hits every leg alike); every leg's first call builds its plans and is not
timed.  Reports the median last_sample_ms per leg and per step, min / max as the run-to-run spread, and the per-forward counts of fused_ip_attn (pairs planned as
one launch) and of pairs left to the plain route.  SD1.5 has 8 heads at every level, so only its 320-wide cross-attentions (d = 40) qualify; all of SDXL's
(d = 64) do.  Appends to profiles/ip_adapter_probe.txt.

usage: ip_adapter_probe.py [steps=20] [reps=5] [models=sd15,sdxl] [out=FILE]"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import sdcpp_amd as sd


def main():
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    steps, reps = int(opts.get("steps", 20)), int(opts.get("reps", 5))
    models = opts.get("models", "sd15,sdxl").split(",")
    path = Path(opts.get("out", ROOT / "profiles" / "ip_adapter_probe.txt"))
    path.parent.mkdir(parents=True, exist_ok=True)
    out = open(path, "a")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    sd.load_mi355x_backend()
    rng = np.random.default_rng(0)
    for tag in models:
        xl = tag == "sdxl"
        t0 = time.time()
        e = sd.Engine(model=sd.SDXL if xl else sd.SD15, wtype=sd.F16, flash_attn=True)
        ctx_dim, batch, px = (2048, 1, 1024) if xl else (768, 8, 512)
        e.ip_adapter_init(ctx_dim, 1280 if xl else 1024, 4, weight_seed=1)
        cond, uncond = (rng.standard_normal((1, 77, ctx_dim)).astype(np.float32) for _ in range(2))
        kw = dict(width=px, height=px, steps=steps, cfg=7.0, seed=42, batch=batch, device_batch=batch, fuse_cfg=True, device_sampler=True, method=sd.EULER_A)
        if xl:
            kw["cond_y"], kw["uncond_y"] = (rng.standard_normal((1, 2816)).astype(np.float32) for _ in range(2))
        tok = {k: (rng.standard_normal((k, ctx_dim)).astype(np.float32), rng.standard_normal((k, ctx_dim)).astype(np.float32)) for k in (4, 16)}
        n_attn2 = sum(1 for nm in e.tensor_names() if nm.endswith("attn2.to_k.weight"))
        say(f"== {'SDXL 1024x1024' if xl else 'SD1.5 512x512'} batch {batch}, {steps} steps, Euler-A, device-resident sampler, {n_attn2} cross-attentions (context made in {time.time() - t0:.0f} s)")

        def leg(n_tok, fused):
            def run():
                sd.backend_set_option("fuse_ip_attn", fused)
                if n_tok:
                    e.set_ip_adapter(tokens=tok[n_tok][0], uncond_tokens=tok[n_tok][1], strength=0.6)
                else:
                    e.set_ip_adapter()
                s0 = sd.backend_stats()
                lat = e.sample_latents(cond, uncond, **kw)
                s1 = sd.backend_stats()
                # fused_ip_attn counts per PLAN: non-zero only in the call that builds the step graph's plan (replays launch without planning)
                return lat, e.stats()["last_sample_ms"], s1["fused_ip_attn"] - s0["fused_ip_attn"]
            return run

        legs = [("adapter off", leg(0, 1)), ("4 tokens, plain nodes", leg(4, 0)), ("4 tokens, fused", leg(4, 1)), ("16 tokens, fused", leg(16, 1))]
        times = {name: [] for name, _ in legs}
        pairs_fused, outs = {}, {}
        for rep in range(reps + 1):   # (an option change drops the cached plans: every timed call follows an untimed one of the same leg, which builds the step graph's plan)
            for name, run in legs:
                _, _, pairs_fused[name] = run()
                outs[name], ms, _ = run()
                if rep > 0:
                    times[name].append(ms)
        for name, _ in legs:
            tt = np.array(times[name])
            pairs = 0 if name == "adapter off" else n_attn2
            say(f"   {name:<24} {np.median(tt):9.2f} ms   ({np.median(tt) / steps:.3f} ms per step; min {tt.min():.2f}, max {tt.max():.2f} over {tt.size} runs; "
                f"per forward: fused pairs {pairs_fused[name]}, plain-route pairs {pairs - pairs_fused[name]})")
        a, b = outs["4 tokens, fused"], outs["4 tokens, plain nodes"]
        say(f"   4 tokens: fused vs plain nodes latents rel-L2 {float(np.linalg.norm(a - b) / np.linalg.norm(b)):.2e}")
        sd.backend_set_option("fuse_ip_attn", 1)
        e.close()


if __name__ == "__main__":
    main()
