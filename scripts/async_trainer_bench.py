#!/usr/bin/env python3
"""HipOffAsyncTrainer against HipOffSerialTrainer on the bench's end-to-end Humanoid loop (bench.py e2e_kwargs: obs 376,
act 17, 3 x 256 nets, batch 256, the table-lookup environment of tests/envs/synth_humanoid_data.py). Needs the GPU.

  python scripts/async_trainer_bench.py [--out profiles] [--pairs 3]
      per configuration (each in a fresh child process) one serial and one async trainer, each with its own handle, then
      `pairs` timing windows of train() alternated between them, with the host time of the loop's phases; configurations: K = 1 and 8 with HipOffSampler, K = 8 with
      HipVecOffSampler N = 64 and N = 256 (GPU route). K = 8 with HipOffSampler also times the async loop with the eager
      live-snapshot copy kept behind every group (debug switch beh_live_copy: what skipping it saves)
  python scripts/async_trainer_bench.py --trace-only
      a short async K = 8 / N = 64 loop (run under rocprofv3 --kernel-trace --stats)
  python scripts/async_trainer_bench.py --analyse-trace KERNEL_TRACE_CSV [--out DIR]
      overlap of the held acting kernels (act_batch_*) with the update kernels in a rocprofv3 kernel trace
Writes DIR/async_trainer_bench.json (or DIR/async_trainer_trace.json) and prints it."""
import argparse
import csv
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
    dict(name="K1_single", K=1, N=0, iters=1200),
    dict(name="K8_single", K=8, N=0, iters=3200, live_copy_leg=True),
    dict(name="K8_vec64_gpu", K=8, N=64, iters=3200),
    dict(name="K8_vec256_gpu", K=8, N=256, iters=1600),
]


def _trainer(cfg, trainer):
    import plugin

    over = dict(sample_interval=cfg["K"], trainer=trainer)
    if cfg["N"]:
        over.update(sampler_name="hip_vec_off_sampler", vector_env_num=cfg["N"], hip_vec_act="gpu",
                    sample_batch_size=cfg["N"], batch_size_per_sampler=cfg["N"])
    kw = bench.e2e_kwargs(HID, bench.B, hip_device=0, **over)
    torch.manual_seed(kw["seed"])
    np.random.seed(kw["seed"])
    alg = plugin.create_alg(**kw)
    sampler = plugin.create_sampler(**kw)
    buf = plugin.create_buffer(**kw)
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
    legs = {"serial": _trainer(cfg, "off_serial_trainer"), "async": _trainer(cfg, "hip_off_async_trainer")}
    if cfg.get("live_copy_leg"):
        legs["async_live_copy"] = _trainer(cfg, "hip_off_async_trainer")
        legs["async_live_copy"][1].engine.debug_set("beh_live_copy", 1)
    phases = {k: {} for k in legs}
    for k, (tr, alg) in legs.items():
        _timed(tr.sampler, "sample", phases[k], "sampler_call")
        _timed(tr.buffer, "add_batch", phases[k], "add_batch")
        _timed(alg, "local_update_group", phases[k], "group_issue")
        if k != "serial":
            _timed(alg, "hold_behaviour", phases[k], "hold")
        _window(tr, alg, warm)
        phases[k].clear()
    rows = {k: [] for k in legs}
    for _ in range(pairs):
        for k, (tr, alg) in legs.items():
            rows[k].append(cfg["iters"] / _window(tr, alg, cfg["iters"]))
    out = {"config": cfg, "iterations_per_s": rows,
           "host_us_per_group": {k: {p: 1e6 * v * cfg["K"] / (pairs * cfg["iters"]) for p, v in ph.items()} for k, ph in phases.items()},
           "us_per_group_median": {k: 1e6 * cfg["K"] / float(np.median(v)) for k, v in rows.items()}}
    for k in legs:
        out[k + "_median"] = float(np.median(rows[k]))
    out["async_over_serial"] = [a / s for a, s in zip(rows["async"], rows["serial"])]
    out["async_over_serial_median"] = float(np.median(out["async_over_serial"]))
    if "async_live_copy" in rows:
        out["async_over_async_live_copy"] = [a / b for a, b in zip(rows["async"], rows["async_live_copy"])]
    e = legs["async"][1].engine
    out["async_holds"] = e.debug_get("beh_holds")
    out["async_held_acts"] = e.debug_get("beh_acts")
    out["handoff_failures"] = {k: alg.engine.debug_get("handoff_failures") for k, (_, alg) in legs.items()}
    for _, alg in legs.values():
        alg.engine.close()
    return out


def trace_only():
    cfg = dict(CONFIGS[2], iters=400)
    tr, alg = _trainer(cfg, "hip_off_async_trainer")
    _window(tr, alg, 80)
    _window(tr, alg, cfg["iters"])
    print("trace-only: done, handoff_failures %d" % alg.engine.debug_get("handoff_failures"))


def analyse_trace(path):
    """the held acting kernels' time that overlaps update kernels (another queue) in a rocprofv3 kernel trace"""
    rows = list(csv.DictReader(open(path)))
    k = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", r.get("Stream_Id", ""))) for r in rows]
    act = [x for x in k if "act_batch" in x[0]]
    upd = sorted([x for x in k if "act_batch" not in x[0]], key=lambda x: x[1])
    starts = np.array([x[1] for x in upd], np.int64)
    ends = np.array([x[2] for x in upd], np.int64)
    tot = ov = n_ov = 0
    for name, s, e, q in act:
        tot += e - s
        i = np.searchsorted(starts, e)
        lo = max(0, i - 4096)
        seg = np.clip(np.minimum(ends[lo:i], e) - np.maximum(starts[lo:i], s), 0, None)
        # union of the overlapping intervals inside [s, e]
        iv = sorted((max(a, s), min(b, e)) for a, b, d in zip(starts[lo:i], ends[lo:i], seg) if d > 0)
        cov, cur_s, cur_e = 0, None, None
        for a, b in iv:
            if cur_e is None or a > cur_e:
                if cur_e is not None:
                    cov += cur_e - cur_s
                cur_s, cur_e = a, b
            else:
                cur_e = max(cur_e, b)
        if cur_e is not None:
            cov += cur_e - cur_s
        ov += cov
        n_ov += cov > 0
    names = sorted({x[0].split("(")[0][:60] for x in act})
    tot, ov, n_ov = int(tot), int(ov), int(n_ov)
    return {"acting_kernels": len(act), "acting_kernels_overlapping_updates": n_ov, "acting_ns": tot, "acting_ns_overlapped": ov,
            "overlap_fraction": ov / tot if tot else None, "update_kernels": len(upd),
            "acting_queues": sorted({x[3] for x in act}), "update_queues": sorted({x[3] for x in upd}), "acting_kernel_names": names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--warm", type=int, default=160)
    ap.add_argument("--only", default="", help="comma-separated configuration names")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--analyse-trace", default="")
    a = ap.parse_args()
    if a.analyse_trace:
        res = analyse_trace(a.analyse_trace)
        print(json.dumps(res, indent=1))
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "async_trainer_trace.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    import __graft_entry__

    __graft_entry__.build()
    if a.trace_only:
        trace_only()
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
    with open(os.path.join(a.out, "async_trainer_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
