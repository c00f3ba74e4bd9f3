"""CPU suite: the N > 1 path (image sharding + result gather) with world_size 2 over gloo on 127.0.0.1, using the CPU
oracle backend on the tiny model.  Sharded results must equal the single-process results image by image."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent

WORKER = r'''
import os, sys, pickle
import numpy as np
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["SD_ROOT"])
import sdcpp_amd as sd
from sdcpp_amd import shard
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{os.environ['MASTER_PORT']}", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
rank, world = dist.get_rank(), dist.get_world_size()
sd.load_backend(os.path.join(os.environ["SD_ROOT"], "oracle/_build/libggml-cpu-oracle.so"))
eng = sd.Engine(model=sd.SD15_TINY, backend="CPU-oracle")
rng = np.random.default_rng(11)
cond = rng.standard_normal((1, 77, 64)).astype(np.float32)
uncond = rng.standard_normal((1, 77, 64)).astype(np.float32)
def gather(local):
    objs = [None] * world
    dist.all_gather_object(objs, local)
    merged = {}
    for o in objs: merged.update(o)
    return merged
res = shard.generate_sharded(eng, cond, uncond, batch_count=5, seed=100, rank=rank, world=world, gather=gather,
                             width=64, height=64, steps=2, cfg=7.0)
dist.barrier()
if rank == 0:
    with open(os.environ["SD_OUT"], "wb") as f: pickle.dump(res, f)
dist.destroy_process_group()
'''


def test_world_size_2_sharding_matches_single_process(sd, oracle, tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = tmp_path / "res.pkl"
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SD_ROOT=str(ROOT), SD_OUT=str(out),
                   OMP_NUM_THREADS="2", OMP_WAIT_POLICY="PASSIVE")
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    import pickle

    res = pickle.loads(out.read_bytes())
    assert sorted(res) == [0, 1, 2, 3, 4]
    from sdcpp_amd import shard

    assert shard.shard_indices(5, 0, 2) == [0, 1, 2] and shard.shard_indices(5, 1, 2) == [3, 4] and shard.shard_indices(2, 3, 4) == []
    eng = sd.Engine(model=sd.SD15_TINY, backend=oracle)
    rng = np.random.default_rng(11)
    cond = rng.standard_normal((1, 77, 64)).astype(np.float32)
    uncond = rng.standard_normal((1, 77, 64)).astype(np.float32)
    ref = eng.sample_latents(cond, uncond, width=64, height=64, steps=2, cfg=7.0, seed=100, batch=5, device_batch=5)
    for b in range(5):
        np.testing.assert_allclose(res[b], ref[b], rtol=1e-4, atol=1e-5)


PAIR_WORKER = r'''
import os, sys, pickle
import numpy as np
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["SD_ROOT"])
import sdcpp_amd as sd
from sdcpp_amd import shard
dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{os.environ['MASTER_PORT']}", rank=int(os.environ["RANK"]), world_size=2)
sd.load_backend(os.path.join(os.environ["SD_ROOT"], "oracle/_build/libggml-cpu-oracle.so"))
eng = sd.Engine(model=sd.SD15_TINY, backend="CPU-oracle")
rng = np.random.default_rng(12)
cond = rng.standard_normal((1, 77, 64)).astype(np.float32)
uncond = rng.standard_normal((1, 77, 64)).astype(np.float32)
out = shard.sample_cfg_pair_split(eng, cond, uncond, width=64, height=64, steps=3, cfg=7.0, seed=77, dist=dist, rank_in_pair=dist.get_rank(), batch=2)
with open(os.environ["SD_OUT"] + str(dist.get_rank()), "wb") as f: pickle.dump(out, f)
dist.barrier()
dist.destroy_process_group()
'''


def test_cfg_pair_split_all_reduce_matches_single_process(sd, oracle, tmp_path):
    """cond on rank 0, uncond on rank 1, one all-reduce of the pre-scaled eps per step (the CFG-pair reduction of SURVEY.md 8(e)):
    both ranks end with the same latents, equal to the single-process Euler-A + CFG trajectory."""
    import pickle

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = tmp_path / "pair.pkl"
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SD_ROOT=str(ROOT), SD_OUT=str(out),
                   OMP_NUM_THREADS="2", OMP_WAIT_POLICY="PASSIVE")
        procs.append(subprocess.Popen([sys.executable, "-c", PAIR_WORKER], env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    a = pickle.loads((tmp_path / "pair.pkl0").read_bytes())
    b = pickle.loads((tmp_path / "pair.pkl1").read_bytes())
    np.testing.assert_array_equal(a, b)
    eng = sd.Engine(model=sd.SD15_TINY, backend=oracle)
    rng = np.random.default_rng(12)
    cond = rng.standard_normal((1, 77, 64)).astype(np.float32)
    uncond = rng.standard_normal((1, 77, 64)).astype(np.float32)
    ref = eng.sample_latents(cond, uncond, width=64, height=64, steps=3, cfg=7.0, seed=77, batch=2, device_batch=2)
    assert float(np.linalg.norm(a - ref) / np.linalg.norm(ref)) < 1e-4


def test_bench_gpus_2_launches_two_ranks():
    """VERDICT r4 task 2: `python bench.py --gpus 2` (the way the driver invokes it, no launcher around it) must run TWO ranks — it re-executes itself under
    torch.distributed.run — and report the ranks that actually took part.  Harness self-check mode: the same launch / shard / reduce code on the CPU oracle
    with gloo (bench.py --selftest-cpu; a GPU run uses RCCL and one MI355X per rank)."""
    import json

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--selftest-cpu", "--full"], capture_output=True, text=True,
                       env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]   # rank 0 alone prints the line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and len(out["ms_per_step_per_rank"]) == 2
    assert out["config"]["global_batch"] == 2 * 2 and out["scaling"] == "weak"
    assert "SELFTEST" in out["metric"]
    # value = all ranks' image-iterations over the slowest rank's time
    assert abs(out["value"] - 4 * out["steps"] / (out["ms_per_step"] * out["steps"] / 1e3)) / out["value"] < 1e-2
    # round 6 (VERDICT r5 missing #5): at N > 1 the line also carries the SDXL leg as it shards (1 image per rank, config 3) and one CFG-pair-split trajectory
    # over the 2-rank group with its exchange timed (here: the tiny UNet over gloo through the same code)
    sh, ps = out["sdxl_sharded"], out["sdxl_cfg_pair_split"]
    assert sh["ranks"] == 2 and sh["steps_timed"] >= 4 and sh["ms_per_step"] > 0 and abs(sh["it_per_s"] - 2 * 1e3 / sh["ms_per_step"]) / sh["it_per_s"] < 1e-2
    assert ps["latents_identical_on_both_ranks"] is True and ps["exchange_us_per_step"] > 0 and ps["ms_per_step"] > 0


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "4", "--selftest-cpu"], capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)
