#!/usr/bin/env python3
"""The vectorised evaluator (training/hip_vec_evaluator.py) against HipEvaluator on the Humanoid 3 x 256 policy with the
table-lookup environment (tests/envs/synth_humanoid_data.py, 1000-step episodes), and dsact_act_mode_batch's two routes.
Needs the GPU.

  python scripts/vec_eval_bench.py --out DIR [--pairs 3]
      eval: run_evaluation wall time, HipEvaluator and HipVecEvaluator alternately in this process, at E = N = 10, 64, 256
      (E = num_eval_episode, N = hip_eval_env_num), plus one CNN row (conv type_2, synth_blob);
      module: per-step cost of HipEvaluator's acting (module forward + dist.mode() + .numpy());
      acting: per-call time of dsact_act_mode_batch on the host route and on the GPU route for n rows -> the crossover
  python scripts/vec_eval_bench.py --kernels-only
      a short stream of GPU-route mode calls only (run under rocprofv3 --kernel-trace --stats)
Writes DIR/vec_eval_bench.json and prints it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dsac-v2_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "envs")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import hip_kwargs  # noqa: E402

HID = (256, 256, 256)
ROWS = (1, 4, 8, 16, 32, 64, 256, 1024)


def humanoid(**over):
    import plugin

    kw = hip_kwargs(376, 17, HID, 256, env_id="synth_humanoid", seed=3, hip_pad_widths=True, **over)
    torch.manual_seed(0)
    return plugin.create_alg(**kw), kw


def evaluators(alg, kw, E, N):
    import plugin

    old = plugin.create_evaluator(**dict(kw, num_eval_episode=E))
    new = plugin.create_evaluator(**dict(kw, num_eval_episode=E, hip_eval_env_num=N))
    old.networks = new.networks = alg.networks
    return old, new


def timed(ev):
    t0 = time.perf_counter()
    tar = ev.run_evaluation(0)
    return time.perf_counter() - t0, float(tar)


def eval_rows(pairs):
    alg, kw = humanoid()
    out = []
    for E in (10, 64, 256):
        old, new = evaluators(alg, kw, E, E)
        assert new.route() == "engine"
        timed(new)   # warm-up: first-call allocations of both routes
        rec = {"E": E, "N": E, "old_s": [], "new_s": [], "old_tar": [], "new_tar": []}
        for _ in range(pairs if E == 10 else 1):
            for name, ev in (("old", old), ("new", new)):
                s, tar = timed(ev)
                rec[name + "_s"].append(s)
                rec[name + "_tar"].append(tar)
        rec["speedup_median"] = float(np.median(rec["old_s"]) / np.median(rec["new_s"]))
        rec["old_us_per_env_step"] = float(np.median(rec["old_s"]) / (E * 1000) * 1e6)
        rec["new_us_per_env_step"] = float(np.median(rec["new_s"]) / (E * 1000) * 1e6)
        rec["old_spread"] = float((max(rec["old_s"]) - min(rec["old_s"])) / np.median(rec["old_s"]))
        rec["new_spread"] = float((max(rec["new_s"]) - min(rec["new_s"])) / np.median(rec["new_s"]))
        out.append(rec)
        print(json.dumps(rec), flush=True)
    return alg, out


def module_step_us(alg, steps=3000):
    """HipEvaluator.run_an_episode's acting, per environment step"""
    obs = np.random.default_rng(0).standard_normal(376).astype(np.float64)
    net = alg.networks
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        with torch.no_grad():
            logits = net.policy(torch.from_numpy(obs.astype("float32")[None]))
            net.create_action_distributions(logits).mode()[0].cpu().numpy()
        t.append(time.perf_counter() - t0)
    return {"median_us": float(np.median(t) * 1e6), "p10_us": float(np.percentile(t, 10) * 1e6),
            "p90_us": float(np.percentile(t, 90) * 1e6)}


def acting_rows(alg, reps=200):
    e = alg.engine
    obs = np.random.default_rng(1).standard_normal((1024, 376)).astype(np.float32)
    act = np.empty((1024, 17), np.float32)
    out = []
    keep = e.debug_get("mode_host_rows")
    for n in ROWS:
        rec = {"n": n}
        for route, rows in (("host", 10 ** 6), ("gpu", 0)):
            e.debug_set("mode_host_rows", rows)
            r = reps if n <= 64 else max(20, reps // 4)
            for _ in range(5):
                e.act_mode_batch_addr(obs.ctypes.data, n, act.ctypes.data)
            t = []
            for _ in range(r):
                t0 = time.perf_counter()
                e.act_mode_batch_addr(obs.ctypes.data, n, act.ctypes.data)
                t.append(time.perf_counter() - t0)
            rec[route + "_us"] = float(np.median(t) * 1e6)
        rec["faster"] = "host" if rec["host_us"] < rec["gpu_us"] else "gpu"
        out.append(rec)
        print(json.dumps(rec), flush=True)
    e.debug_set("mode_host_rows", keep)
    return out


def cnn_row(E=10):
    import plugin
    from test_hip_cnn_parity import cnn_kwargs

    kw = cnn_kwargs((3, 96, 96), 3, "type_2", 8, env_id="synth_blob", seed=4, strict_rng=False)
    torch.manual_seed(0)
    alg = plugin.create_alg(**kw)
    old, new = evaluators(alg, kw, E, E)
    assert new.route() == "engine"
    timed(new)
    rec = {"E": E, "N": E, "episode_steps": 20, "old_s": [], "new_s": []}
    for _ in range(2):
        for name, ev in (("old", old), ("new", new)):
            rec[name + "_s"].append(timed(ev)[0])
    rec["speedup_median"] = float(np.median(rec["old_s"]) / np.median(rec["new_s"]))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if a.kernels_only:
        alg, _ = humanoid()
        e = alg.engine
        e.debug_set("mode_host_rows", 0)
        obs = np.random.default_rng(1).standard_normal((256, 376)).astype(np.float32)
        for n in (1, 10, 64, 256):
            for _ in range(50):
                e.act_mode_batch(obs[:n])
        print("kernels-only: done")
        return
    alg, ev = eval_rows(a.pairs)
    res = {"device": torch.cuda.get_device_name(0), "policy": "Humanoid 376 -> 3 x 256 -> 17 (hip_pad_widths)",
           "env": "tests/envs/synth_humanoid_data.py (1000-step episodes)", "eval": ev,
           "module_forward_step": module_step_us(alg), "act_mode_batch": acting_rows(alg), "cnn_type2_synth_blob": cnn_row()}
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "vec_eval_bench.json"), "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
