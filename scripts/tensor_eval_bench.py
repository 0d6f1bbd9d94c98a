#!/usr/bin/env python3
"""The device-resident evaluator (evaluator_name="hip_tensor_env_evaluator") against HipVecEvaluator on the
SAME dynamics: tests/envs/synth_tensor_humanoid.py (obs 376, act 17, 1000-step limit) as one batched environment on the GPU for
the new route, and as N per-environment objects (the adapter of scripts/tensor_sampler_bench.py, restarted from the first state
for every episode so that both legs play the same N episodes) for the baseline. The policy is the bench's Humanoid
configuration (3 x 256, untrained). E = N episodes: every environment plays one. Needs the GPU.

  python scripts/tensor_eval_bench.py [--out profiles] [--pairs 3]
      per N in 64, 256, 1024 (each in a fresh child process under a time limit): wall time of run_evaluation(), the engine's
        stream drained at both ends; one warm-up evaluation per leg, then `pairs` alternating (tensor, vec) pairs. The tensor
        leg repeats the evaluation inside a window until about --window seconds have passed (every repetition is the same work).
      the poll period (one more child process): hip_eval_poll_steps P in 1, 4, 16, 64 at N = 256, the four periods taken in turn
        inside each of `pairs` rounds.
      Medians, per-pair ratios (vec / tensor) and each leg's spread over its own windows are recorded.
Writes DIR/tensor_eval_bench.json and prints it. The library must have been built (__graft_entry__.build())."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dsac-v2_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "envs"),
          os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import hip_kwargs  # noqa: E402
from synth_tensor_humanoid import A, O, SynthTensorHumanoid  # noqa: E402
from tensor_sampler_bench import OneEnv  # noqa: E402

NS = [64, 256, 1024]
PS = [1, 4, 16, 64]
HID, B, SEED, LIMIT = (256, 256, 256), 256, 3, 1000


class FreshEnv(OneEnv):
    """every episode starts from the environment's first state, like the batched environment's reset()"""

    def reset(self):
        return self.env.reset()[0].numpy(), {}


def _alg():
    import plugin

    kw = hip_kwargs(O, A, HID, B, seed=SEED, strict_rng=False, hip_pad_widths=True)
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    return plugin.create_alg(**kw)


def _tensor(alg, N, P=None):
    import plugin

    kw = {} if P is None else {"hip_eval_poll_steps": P}
    return plugin.create_evaluator(evaluator_name="hip_tensor_env_evaluator", networks=alg.networks, num_eval_episode=N,
                                   eval_env=SynthTensorHumanoid(N, device="cuda", seed=SEED, episode_limit=LIMIT), **kw)


def _vec(alg, N):
    import plugin

    envs = [FreshEnv(i) for i in range(N)]
    for e in envs:
        e.env.episode_limit[:] = LIMIT
    return plugin.create_evaluator(hip_eval_env_num=N, eval_envs=envs, networks=alg.networks, num_eval_episode=N)


def _window(alg, ev, reps):
    """seconds per run_evaluation over `reps` repetitions, the stream drained at both ends; the last TAR"""
    alg.engine.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        tar = ev.run_evaluation(0)
    alg.engine.sync()
    return (time.perf_counter() - t0) / reps, float(tar)


def _stats(rows):
    return {"median": {k: float(np.median(v)) for k, v in rows.items()},
            "spread": {k: (max(v) - min(v)) / float(np.median(v)) for k, v in rows.items()}}


def run_n(N, pairs, window):
    alg = _alg()
    legs = {"tensor": _tensor(alg, N), "vec": _vec(alg, N)}
    reps, tars = {}, {}
    for leg, ev in legs.items():                      # warm-up; the tensor leg's time sizes its windows
        dt, tars[leg] = _window(alg, ev, 1)
        if leg == "tensor":
            dt, _ = _window(alg, ev, 1)
        reps[leg] = max(1, int(round(window / dt))) if leg == "tensor" else 1
    rows = {leg: [] for leg in legs}
    for _ in range(pairs):
        for leg, ev in legs.items():
            rows[leg].append(_window(alg, ev, reps[leg])[0])
    ratios = [v / t for t, v in zip(rows["tensor"], rows["vec"])]
    e = alg.engine
    out = {"N": N, "episodes": N, "metric": "seconds_per_run_evaluation", "repetitions_per_window": reps, "rows": rows,
           "vec_over_tensor": ratios, "vec_over_tensor_median": float(np.median(ratios)),
           "lockstep_steps": {k: int(ev.steps) for k, ev in legs.items()}, "tar": tars,
           "mean_episode_length": float(np.mean(legs["tensor"].lengths)), "poll_steps": legs["tensor"].poll_steps,
           "act_dev_syncs": e.debug_get("act_dev_syncs"), "handoff_failures": e.debug_get("handoff_failures")}
    out.update(_stats(rows))
    e.close()
    return out


def run_poll(N, pairs, window):
    alg = _alg()
    legs = {P: _tensor(alg, N, P) for P in PS}
    reps = {}
    for P, ev in legs.items():
        _window(alg, ev, 1)
        reps[P] = max(1, int(round(window / _window(alg, ev, 1)[0])))
    rows = {P: [] for P in PS}
    for _ in range(pairs):
        for P, ev in legs.items():
            rows[P].append(_window(alg, ev, reps[P])[0])
    out = {"N": N, "episodes": N, "metric": "seconds_per_run_evaluation", "repetitions_per_window": reps,
           "rows": {str(P): v for P, v in rows.items()}, "lockstep_steps": {str(P): int(ev.steps) for P, ev in legs.items()}}
    out.update(_stats({str(P): v for P, v in rows.items()}))
    alg.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--only", default="", help="N or poll:N -- one configuration, in this process")
    a = ap.parse_args()
    if a.only:
        r = run_poll(int(a.only[5:]), a.pairs, a.window) if a.only.startswith("poll:") else run_n(int(a.only), a.pairs, a.window)
        print("RESULT " + json.dumps(r), flush=True)
        return
    res = {"pairs": a.pairs, "window_s": a.window, "policy": "376-256-256-256-34", "episode_limit": LIMIT, "configs": [], "poll": None}
    for only in [str(n) for n in NS] + ["poll:256"]:
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--only", only, "--pairs", str(a.pairs),
               "--window", str(a.window)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("configuration %s failed (exit status %d)" % (only, p.returncode))
        r = json.loads(line[-1][len("RESULT "):])
        if only.startswith("poll:"):
            res["poll"] = r
        else:
            res["configs"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "tensor_eval_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
