#!/usr/bin/env python3
"""What the episode statistics of the device-resident sampler cost (hip_episode_stats): sampler-only
environment steps / s of HipTensorEnvSampler.sample() on tests/envs/synth_tensor_humanoid.py (obs 376, act 17; the bench's
3 x 256 policy) with the statistics OFF against ON (hip_episode_stats_every = 0: one more launch per sample(), no read), in the
manner of scripts/tensor_sampler_bench.py. Needs the GPU.

  python scripts/tensor_sampler_stats_bench.py [--out profiles] [--pairs 3] [--window 0.6]
      per N in 64, 4096 and per S in N (one lockstep step per sample(): the worst case, one extra launch per step) and 8 N,
      each configuration in a fresh child process: both samplers on ONE engine (each with its own environment instance), one
      warm-up window per leg (which also sizes the windows to about --window seconds), then `pairs` alternating pairs of windows,
      the stream drained at both ends of a window. Medians, per-pair ratios (on / off) and each leg's spread over its own
      windows are recorded.
Writes DIR/tensor_sampler_stats_bench.json and prints it. The library must have been built (__graft_entry__.build())."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dsac-v2_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "envs")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import hip_kwargs  # noqa: E402
from synth_tensor_humanoid import A, O, SynthTensorHumanoid  # noqa: E402

NS, MULTS = [64, 4096], [1, 8]
HID, B, SEED = (256, 256, 256), 256, 3


def _window(eng, smp, count):
    """`count` sample() calls; seconds, the stream drained at both ends"""
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(count):
        smp.sample()
    eng.sync()
    return time.perf_counter() - t0


def run(N, mult, pairs, window):
    import plugin

    S = N * mult
    kw = hip_kwargs(O, A, HID, B, seed=SEED, sample_batch_size=S, buffer_max_size=max(100_000, 4 * S), strict_rng=False,
                    hip_pad_widths=True)
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    alg = plugin.create_alg(**kw)
    eng = alg.engine
    legs = {}
    for leg, over in (("off", {}), ("on", {"hip_episode_stats": True, "hip_episode_stats_every": 0})):
        legs[leg] = plugin.create_sampler(sampler_name="hip_tensor_env_sampler", env=SynthTensorHumanoid(N, device="cuda", seed=SEED),
                                          networks=alg.networks, **dict(kw, **over))
    counts = {}
    for leg, smp in legs.items():                    # warm-up; its rate sizes the windows
        dt = _window(eng, smp, 4)
        dt = _window(eng, smp, 4)
        counts[leg] = max(4, int(round(window / (dt / 4))))
    n = counts["on"] = counts["off"] = min(counts.values())     # the two legs run windows of the same length
    rows = {leg: [] for leg in legs}
    for _ in range(pairs):
        for leg, smp in legs.items():
            rows[leg].append(n * S / _window(eng, smp, n))
    ratios = [a / b for a, b in zip(rows["on"], rows["off"])]
    stats = legs["on"].episode_statistics(clear=False)
    out = {"N": N, "S": S, "metric": "env_steps_per_s", "window_calls": n, "rows": rows,
           "median": {k: float(np.median(v)) for k, v in rows.items()},
           "on_over_off": ratios, "on_over_off_median": float(np.median(ratios)),
           "spread": {k: (max(v) - min(v)) / float(np.median(v)) for k, v in rows.items()},
           "episodes_tracked": stats["episodes"], "track_commit_calls": eng.debug_get("track_commit_calls"),
           "track_reads": eng.debug_get("track_reads"), "act_dev_syncs": eng.debug_get("act_dev_syncs"),
           "handoff_failures": eng.debug_get("handoff_failures")}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.6)
    ap.add_argument("--only", default="", help="N:mult -- one configuration, in this process")
    a = ap.parse_args()
    if a.only:
        n, mult = a.only.split(":")
        print("RESULT " + json.dumps(run(int(n), int(mult), a.pairs, a.window)), flush=True)
        return
    res = {"pairs": a.pairs, "window_s": a.window, "policy": "376-256-256-256-34", "configs": []}
    for n in NS:
        for mult in MULTS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "%d:%d" % (n, mult), "--pairs", str(a.pairs),
                                "--window", str(a.window)], capture_output=True, text=True, timeout=240)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("configuration %d:%d failed (exit status %d)" % (n, mult, p.returncode))
            r = json.loads(line[-1][len("RESULT "):])
            res["configs"].append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "tensor_sampler_stats_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
