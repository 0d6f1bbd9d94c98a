#!/usr/bin/env python3
"""The vectorised sampler (training/hip_vec_sampler.py) against HipOffSampler on the bench's end-to-end Humanoid loop
(bench.py e2e_kwargs: obs 376, act 17, 3 x 256 policy, table-lookup environment), and the batched acting call
(dsact_act_sample_batch) against N per-row host calls (dsact_act_sample). Needs the GPU.

  python scripts/vec_sampler_bench.py --out DIR [--envs 1,4,16,64,256] [--iters 300] [--rounds 2]
      e2e: per round, for every N, the HipOffSampler loop and the HipVecOffSampler loop alternately in this process;
      acting: time per lockstep step of the batched call vs N x the per-row call, and the crossover
  python scripts/vec_sampler_bench.py --kernels-only
      a short stream of batched acting calls only (run under rocprofv3 --kernel-trace --stats)
Writes DIR/vec_sampler_bench.json and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dsac-v2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (e2e_kwargs, _timed_loop: the bench's own loop)

HID = (256, 256, 256)


def e2e(n_envs, iters, warm):
    """iterations/s and environment steps/s of HipOffSerialTrainer.step() with one sampler call per update"""
    import plugin

    S = max(1, n_envs) * -(-20 // max(1, n_envs))   # the bench's 20 environment steps per iteration, rounded up to a multiple of N
    over = {"sample_batch_size": S, "batch_size_per_sampler": S}
    if n_envs:
        over.update(sampler_name="hip_vec_off_sampler", vector_env_num=n_envs)
    kw = bench.e2e_kwargs(HID, bench.B, hip_device=0, **over)
    torch.manual_seed(kw["seed"])
    np.random.seed(kw["seed"])
    alg = plugin.create_alg(**kw)
    sampler = plugin.create_sampler(**kw)
    buf = plugin.create_buffer(**kw)
    trainer = plugin.create_trainer(alg, sampler, buf, None, **kw)
    w, ws = bench._timed_loop(trainer, sampler, warm, iters, alg.engine.sync)
    route = sampler.route() if n_envs else "HipOffSampler"
    alg.engine.close()
    return {"sampler": "HipVecOffSampler" if n_envs else "HipOffSampler", "N": n_envs or 1, "route": route,
            "env_steps_per_iteration": S, "iterations_per_s": iters / w, "env_steps_per_s": S * iters / w,
            "ms_per_iteration": 1e3 * w / iters, "sampler_ms_per_iteration": 1e3 * ws / iters,
            "sampler_us_per_env_step": 1e6 * ws / (iters * S)}


def acting(ns, reps=300):
    """host wall time of ONE batched call for N rows vs N per-row calls (the host acting forward), same weights"""
    import plugin

    kw = bench.e2e_kwargs(HID, bench.B, hip_device=0)
    alg = plugin.create_alg(**kw)
    e = alg.engine
    A, O = e.act_dim, e.obs_dim
    rng = np.random.default_rng(0)
    rows = []
    for n in ns:
        obs = rng.standard_normal((n, O)).astype(np.float32)
        eps = rng.standard_normal((n, A)).astype(np.float32)
        act = np.empty((n, A), np.float32)
        lp = np.empty(n, np.float32)
        oa, ea, aa, la = obs.ctypes.data, eps.ctypes.data, act.ctypes.data, lp.ctypes.data
        r = max(20, reps // max(1, n // 16))

        def batched():
            e.act_sample_batch_addr(oa, n, ea, aa, la)

        def per_row():
            for i in range(n):
                e.act_sample_addr(oa + 4 * O * i, ea + 4 * A * i, aa + 4 * A * i, la + 4 * i)

        out = {"N": n}
        for name, f in (("gpu_batch_us", batched), ("host_rows_us", per_row), ("gpu_batch_us_2", batched), ("host_rows_us_2", per_row)):
            for _ in range(10):
                f()
            t0 = time.perf_counter()
            for _ in range(r):
                f()
            out[name] = 1e6 * (time.perf_counter() - t0) / r
        out["gpu_batch_us"] = min(out.pop("gpu_batch_us_2"), out["gpu_batch_us"])
        out["host_rows_us"] = min(out.pop("host_rows_us_2"), out["host_rows_us"])
        out["host_per_row_us"] = out["host_rows_us"] / n
        out["gpu_per_row_us"] = out["gpu_batch_us"] / n
        rows.append(out)
    cross = next((r["N"] for r in rows if r["gpu_batch_us"] < r["host_rows_us"]), None)
    alg.engine.close()
    return {"rows": rows, "crossover_N": cross}


def kernels_only():
    import plugin

    kw = bench.e2e_kwargs(HID, bench.B, hip_device=0)
    alg = plugin.create_alg(**kw)
    e = alg.engine
    rng = np.random.default_rng(0)
    for n in (16, 64, 256, 1024):
        obs = rng.standard_normal((n, e.obs_dim)).astype(np.float32)
        eps = rng.standard_normal((n, e.act_dim)).astype(np.float32)
        for _ in range(50):
            e.act_sample_batch(obs, eps)
    e.sync()
    print("kernels-only: done")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=".", help="directory for vec_sampler_bench.json (default: the current one)")
    ap.add_argument("--envs", default="1,4,16,64,256")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    if a.kernels_only:
        kernels_only()
        return
    res = {"acting": acting([1, 2, 4, 8, 12, 16, 32, 64, 128, 256, 1024]), "e2e": []}
    print(json.dumps(res["acting"]), flush=True)
    for rnd in range(a.rounds):
        for n in [int(v) for v in a.envs.split(",")]:
            for which in (0, n):        # alternated: the one-environment loop, then the vectorised one
                r = e2e(which, a.iters, a.warm)
                r["round"] = rnd
                res["e2e"].append(r)
                print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "vec_sampler_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
