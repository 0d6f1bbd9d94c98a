#!/usr/bin/env python3
"""Device-drawn replay indices (`hip_device_indices=True`) against the default host draw
(np.random.randint + pinned staging + upload) on the bench's end-to-end Humanoid loop (bench.py e2e_kwargs: obs 376, act 17,
3 x 256 nets, batch 256, the table-lookup environment of tests/envs/synth_humanoid_data.py). Needs the GPU.

  python scripts/device_indices_bench.py [--out profiles] [--pairs 3]
      per configuration (each in a fresh child process) one trainer with host indices and one with device indices, each with
      its own handle, then `pairs` timing windows of train() alternated between them, with the host time of the loop's
      phases. Configurations: serial K = 1, serial K = 8, async K = 8 with HipOffSampler, async K = 8 with HipVecOffSampler
      N = 64 (GPU route).
  python scripts/device_indices_bench.py --trace-only host|device
      a short serial K = 8 loop of that leg (run under rocprofv3 --kernel-trace --stats, one run per leg)
Writes DIR/device_indices_bench.json and prints it."""
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

import bench  # noqa: E402  (e2e_kwargs: the bench's own configuration)

HID = (256, 256, 256)
CONFIGS = [
    dict(name="serial_K1", trainer="off_serial_trainer", K=1, N=0, iters=1200),
    dict(name="serial_K8", trainer="off_serial_trainer", K=8, N=0, iters=3200),
    dict(name="async_K8_single", trainer="hip_off_async_trainer", K=8, N=0, iters=3200),
    dict(name="async_K8_vec64_gpu", trainer="hip_off_async_trainer", K=8, N=64, iters=3200),
]
LEGS = {"host": False, "device": True}


def _trainer(cfg, device_indices):
    import plugin

    over = dict(sample_interval=cfg["K"], trainer=cfg["trainer"], hip_device_indices=device_indices)
    if cfg["N"]:
        over.update(sampler_name="hip_vec_off_sampler", vector_env_num=cfg["N"], hip_vec_act="gpu",
                    sample_batch_size=cfg["N"], batch_size_per_sampler=cfg["N"])
    kw = bench.e2e_kwargs(HID, bench.B, hip_device=0, **over)
    torch.manual_seed(kw["seed"])
    np.random.seed(kw["seed"])
    alg = plugin.create_alg(**kw)
    sampler = plugin.create_sampler(**kw)
    buf = plugin.create_buffer(**kw)
    assert buf.engine is alg.engine and buf.device_indices == device_indices
    tr = plugin.create_trainer(alg, sampler, buf, None, **dict(kw, max_iteration=0))
    if cfg["N"]:
        assert sampler.route() == "gpu", sampler.route()
    return tr, alg


def _timed(obj, name, acc, key):
    inner = getattr(obj, name)

    def f(*a, **k):
        t0 = time.perf_counter()
        r = inner(*a, **k)
        acc[key] = acc.get(key, 0.0) + time.perf_counter() - t0
        return r

    setattr(obj, name, f)


def _window(tr, alg, iters):
    """iters more iterations of train(); returns seconds"""
    alg.engine.sync()
    tr.max_iteration = tr.iteration + iters
    t0 = time.perf_counter()
    tr.train()
    alg.engine.sync()
    return time.perf_counter() - t0


def run_config(cfg, pairs, warm):
    legs = {k: _trainer(cfg, v) for k, v in LEGS.items()}
    phases = {k: {} for k in legs}
    for k, (tr, alg) in legs.items():
        _timed(tr.sampler, "sample", phases[k], "sampler_call")
        _timed(tr.buffer, "add_batch", phases[k], "add_batch")
        _timed(tr.buffer, "sample_batches" if cfg["K"] > 1 else "sample_batch", phases[k], "index_draw")
        _timed(alg, "local_update_group" if cfg["K"] > 1 else "local_update", phases[k], "update_issue")
        if hasattr(tr, "_hold"):
            _timed(alg, "hold_behaviour", phases[k], "hold")
        _window(tr, alg, warm)
        phases[k].clear()
    rows = {k: [] for k in legs}
    for _ in range(pairs):
        for k, (tr, alg) in legs.items():
            rows[k].append(cfg["iters"] / _window(tr, alg, cfg["iters"]))
    ratios = [d / h for d, h in zip(rows["device"], rows["host"])]
    out = {"config": cfg, "iterations_per_s": rows,
           "host_us_per_group": {k: {p: 1e6 * v * cfg["K"] / (pairs * cfg["iters"]) for p, v in ph.items()} for k, ph in phases.items()},
           "us_per_group_median": {k: 1e6 * cfg["K"] / float(np.median(v)) for k, v in rows.items()},
           "device_over_host": ratios, "device_over_host_median": float(np.median(ratios)),
           # the spread of one leg over its own windows: what a difference between the legs has to exceed
           "pair_spread": {k: (max(v) - min(v)) / float(np.median(v)) for k, v in rows.items()},
           "handoff_failures": {k: alg.engine.debug_get("handoff_failures") for k, (_, alg) in legs.items()}}
    for k in legs:
        out[k + "_median"] = float(np.median(rows[k]))
    for _, alg in legs.values():
        alg.engine.close()
    return out


def trace_only(leg):
    cfg = dict(CONFIGS[1], iters=800)
    tr, alg = _trainer(cfg, LEGS[leg])
    _window(tr, alg, 80)
    _window(tr, alg, cfg["iters"])
    print("trace-only: %s indices done, handoff_failures %d" % (leg, alg.engine.debug_get("handoff_failures")))
    alg.engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--warm", type=int, default=160)
    ap.add_argument("--only", default="", help="comma-separated configuration names")
    ap.add_argument("--trace-only", default="", choices=["", "host", "device"])
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    if a.trace_only:
        trace_only(a.trace_only)
        return
    if a.only and "," not in a.only:      # one configuration, in this process
        r = run_config(next(c for c in CONFIGS if c["name"] == a.only), a.pairs, a.warm)
        print("RESULT " + json.dumps(r), flush=True)
        return
    import subprocess

    res = {"pairs": a.pairs, "configs": []}
    for cfg in CONFIGS:
        if a.only and cfg["name"] not in a.only.split(","):
            continue
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", cfg["name"], "--pairs", str(a.pairs),
                            "--warm", str(a.warm)], capture_output=True, text=True, timeout=600)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("configuration %s failed (exit status %d)" % (cfg["name"], p.returncode))
        r = json.loads(line[-1][len("RESULT "):])
        res["configs"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "device_indices_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
