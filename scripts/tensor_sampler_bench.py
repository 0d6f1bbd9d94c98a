#!/usr/bin/env python3
"""The device-resident sampler (sampler_name="hip_tensor_env_sampler") against HipVecOffSampler's GPU route
on the SAME dynamics: tests/envs/synth_tensor_humanoid.py (obs 376, act 17) as one batched environment on the GPU for the new
route, and as N per-environment objects (environment i alone on the CPU device, behind the gym-0.23 face HipVecOffSampler
steps) for the baseline. Policy and update are the bench's Humanoid configuration (3 x 256 nets, batch 256). Needs the GPU.

  python scripts/tensor_sampler_bench.py [--out profiles] [--pairs 3] [--window 0.6]
      per N in 64, 256, 1024, 4096 (each in a fresh child process) and per metric
        sampler: environment steps / s of sample() alone (one lockstep step per call, the stream drained at the window's end)
        trainer: iterations / s of HipOffSerialTrainer at sample_interval K = 8, hip_device_indices=True
      one warm-up window per leg (which also sizes the windows to about --window seconds), then `pairs` alternating pairs of
      windows. Medians, per-pair ratios (tensor / vec) and each leg's spread over its own windows are recorded.
  python scripts/tensor_sampler_bench.py --noise [--noise-n 1024] [--out profiles] [--pairs 3] [--window 0.6]
      opt-in: the sampler-only metric of the tensor route alone, without and with
      noise_params={"mean": 0.0, "std": 0.1} (the exploration noise drawn in the acting kernel), both legs in ONE fresh child
      process with alternating windows. Writes DIR/explore_noise_bench.json; nothing else is run.
  python scripts/tensor_sampler_bench.py --graph [--tree DIR] [--out profiles] [--pairs 3] [--window 0.6]
      opt-in: the tensor route issued eagerly against the same route with hip_graph_sample=True (sample()
      as one captured graph, on tests/envs/synth_tensor_humanoid_inplace.py), N in 64, 256, 1024, each configuration in a fresh
      child process with alternating windows: `sampler` (environment steps / s of sample() alone), `trainer1` / `trainer8`
      (iterations / s of HipOffSerialTrainer at sample_interval 1 / 8), and `rows`: a hip_graph_sample sampler held on its eager
      route, its row copies as one launch (dsact_step_rows_device) against the torch copies. --tree DIR runs the EAGER leg alone
      with the package, helpers and fixtures of another checkout (DIR/dsac-v2_amd with its built library, DIR/tests): the parent
      commit's numbers, recorded as "parent_eager" beside the others (DIR = this checkout: "eager_alone", the same process
      layout on this tree -- a leg that shares its process with a second engine issues its launches about a tenth slower). Writes DIR/graph_sample_bench.json; nothing else is run.
  python scripts/tensor_sampler_bench.py --wrap none torch fused [--graph] [--out profiles] [--pairs 3] [--window 0.6]
      opt-in: sample() alone at S = N, N in 64, 1024, with the reference's three environment wrappers
      (training/hip_tensor_env_wrappers.py: max_episode_steps=1000, reward shift and scale, a per-element observation shift and
      scale) on the torch route / on the fused route (one launch behind step and reset each), against `none`: the bare
      environment, whose own limit is the same 1000 steps. The legs named share ONE fresh child process per N with alternating
      windows; --graph: every leg with hip_graph_sample=True on the in-place fixture. Recorded per leg: environment steps / s and
      the library's launches per lockstep step from the debug counters (act_dev_calls, step_rows_calls, env_wrap_calls; torch's
      own launches are not counted there). Writes DIR/env_wrap_bench.json ("eager" / "graph"); nothing else is run.
Writes DIR/tensor_sampler_bench.json and prints it. The library must have been built (__graft_entry__.build())."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_ROOT = ROOT
if "--tree" in sys.argv:             # (before the imports below: they come from that checkout)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
for p in (ROOT, os.path.join(ROOT, "dsac-v2_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "envs")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import hip_kwargs  # noqa: E402
from synth_humanoid_data import _Box  # noqa: E402
from synth_tensor_humanoid import ACT_LIMIT, A, O, SynthTensorHumanoid  # noqa: E402

NS = [64, 256, 1024, 4096]
HID, B, K, SEED = (256, 256, 256), 256, 8, 3


class OneEnv:
    """environment i of the batched fixture on its own, with the interface HipVecOffSampler steps"""

    pool = None

    def __init__(self, i):
        self.env = SynthTensorHumanoid(1, seed=SEED, env_offset=i, pool=OneEnv.pool)
        OneEnv.pool = self.env.pool     # one pool for the N objects
        self.action_space = _Box(np.full(A, -ACT_LIMIT), np.full(A, ACT_LIMIT))
        self.started = False
        self.all = torch.ones(1, dtype=torch.bool)

    def reset(self):
        obs = self.env.reset(self.all) if self.started else self.env.reset()
        self.started = True
        return obs[0].numpy(), {}

    def step(self, a):
        o2, r, te, tr = self.env.step(torch.from_numpy(np.asarray(a, np.float32).reshape(1, A)))
        return o2[0].numpy(), float(r), bool(te), {"TimeLimit.truncated": bool(tr)}


NOISE = {"mean": 0.0, "std": 0.1}


def _leg(leg, N, trainer):
    """leg: "tensor" | "vec"; "noise": the tensor leg with noise_params=NOISE"""
    import plugin

    kw = hip_kwargs(O, A, HID, B, seed=SEED, sample_batch_size=N, buffer_max_size=max(100_000, 4 * N), buffer_warm_size=max(B, N),
                    sample_interval=K, max_iteration=0, log_save_interval=10 ** 9, apprfunc_save_interval=10 ** 9, eval_interval=10 ** 9,
                    save_folder=None, ini_network_dir=None, strict_rng=False, hip_device_indices=True, hip_pad_widths=True)
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    alg = plugin.create_alg(**kw)
    if leg in ("tensor", "noise"):
        smp = plugin.create_sampler(sampler_name="hip_tensor_env_sampler", env=SynthTensorHumanoid(N, device="cuda", seed=SEED),
                                    **dict(kw, noise_params=NOISE if leg == "noise" else None))
    else:
        smp = plugin.create_sampler(sampler_name="hip_vec_off_sampler", envs=[OneEnv(i) for i in range(N)], hip_vec_act="gpu", **kw)
    smp.networks = alg.networks
    tr = None
    if trainer:
        buf = plugin.create_buffer(**kw)
        tr = plugin.create_trainer(alg, smp, buf, None, **kw)
    if leg == "vec":
        assert smp.route() == "gpu", smp.route()
    return alg, smp, tr


def _window(alg, smp, tr, count, hold_eager=False):
    """`count` sample() calls, or `count` trainer iterations; seconds, the stream drained at both ends. hold_eager: a
    hip_graph_sample sampler is kept on its first (eager) call"""
    alg.engine.sync()
    t0 = time.perf_counter()
    if tr is None:
        for _ in range(count):
            if hold_eager:
                smp._graph_calls = 0
            smp.sample()
    else:
        tr.max_iteration = tr.iteration + count
        tr.train()
    alg.engine.sync()
    return time.perf_counter() - t0


def run(N, metric, pairs, window):
    trainer = metric == "trainer"
    unit = K if trainer else 1
    other = "noise" if metric == "noise" else "vec"      # metric "noise": sample() alone, the tensor route without / with noise
    legs = {leg: _leg(leg, N, trainer) for leg in ("tensor", other)}
    counts = {}
    for leg, h in legs.items():                      # warm-up; its rate sizes the windows
        c = 2 * unit
        dt = _window(*h, c)
        dt = _window(*h, c)
        counts[leg] = max(2 * unit, int(round(window / (dt / c) / unit)) * unit)
    rows = {leg: [] for leg in legs}
    for _ in range(pairs):
        for leg, h in legs.items():
            dt = _window(*h, counts[leg])
            rows[leg].append(counts[leg] * (1 if trainer else N) / dt)
    ratios = [t / v for t, v in zip(rows["tensor"], rows[other])]
    out = {"N": N, "metric": "iterations_per_s" if trainer else "env_steps_per_s", "window_counts": counts, "rows": rows,
           "median": {k: float(np.median(v)) for k, v in rows.items()},
           "tensor_over_" + other: ratios, "tensor_over_%s_median" % other: float(np.median(ratios)),
           "spread": {k: (max(v) - min(v)) / float(np.median(v)) for k, v in rows.items()},
           "act_dev_syncs": legs["tensor"][0].engine.debug_get("act_dev_syncs"),
           "handoff_failures": {k: h[0].engine.debug_get("handoff_failures") for k, h in legs.items()}}
    if other == "noise":
        out["noise_params"] = NOISE
        out["explore_noise"] = {k: h[0].engine.debug_get("explore_noise") for k, h in legs.items()}
    for h in legs.values():
        h[0].engine.close()
    return out


GRAPH_NS = [64, 256, 1024]
GRAPH_METRICS = ("sampler", "trainer1", "trainer8", "rows")


def _graph_leg(leg, N, k):
    """leg: "eager" (the plain tensor route) | "graph" (hip_graph_sample=True) | "rows" / "torch" (hip_graph_sample=True held on
    its eager route, the row copies as one launch / as torch copies). k: sample_interval of a trainer, 0: sample() alone"""
    import plugin

    kw = hip_kwargs(O, A, HID, B, seed=SEED, sample_batch_size=N, buffer_max_size=max(100_000, 4 * N), buffer_warm_size=max(B, N),
                    sample_interval=max(k, 1), max_iteration=0, log_save_interval=10 ** 9, apprfunc_save_interval=10 ** 9,
                    eval_interval=10 ** 9, save_folder=None, ini_network_dir=None, strict_rng=False, hip_device_indices=True,
                    hip_pad_widths=True)
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    alg = plugin.create_alg(**kw)
    if leg == "eager":
        env, more = SynthTensorHumanoid(N, device="cuda", seed=SEED), {}
    else:
        from synth_tensor_humanoid_inplace import SynthTensorHumanoidInplace
        env, more = SynthTensorHumanoidInplace(N, device="cuda", seed=SEED), {"hip_graph_sample": True}
    smp = plugin.create_sampler(**dict(kw, sampler_name="hip_tensor_env_sampler", env=env, **more))
    smp.networks = alg.networks
    if leg == "torch":
        smp._one_launch_rows = False
    tr = None
    if k:
        buf = plugin.create_buffer(**kw)
        tr = plugin.create_trainer(alg, smp, buf, None, **kw)
    return alg, smp, tr


def run_graph(N, metric, pairs, window, parent):
    k = {"sampler": 0, "rows": 0, "trainer1": 1, "trainer8": 8}[metric]
    names = ("eager",) if parent else ("rows", "torch") if metric == "rows" else ("eager", "graph")
    legs = {leg: _graph_leg(leg, N, k) for leg in names}
    hold = metric == "rows"
    unit = k or 1
    counts = {}
    for leg, h in legs.items():                      # warm-up (eager call, capture, replays); its rate sizes the windows
        c = 4 * unit
        dt = _window(*h, c, hold)
        dt = _window(*h, c, hold)
        counts[leg] = max(4 * unit, int(round(window / (dt / c) / unit)) * unit)
    rows = {leg: [] for leg in legs}
    for _ in range(pairs):
        for leg, h in legs.items():
            dt = _window(*h, counts[leg], hold)
            rows[leg].append(counts[leg] * (N if not k else 1) / dt)
    out = {"N": N, "metric": metric, "unit": "iterations_per_s" if k else "env_steps_per_s", "window_counts": counts, "rows": rows,
           "median": {x: float(np.median(v)) for x, v in rows.items()},
           "spread": {x: (max(v) - min(v)) / float(np.median(v)) for x, v in rows.items()},
           "act_dev_syncs": {x: h[0].engine.debug_get("act_dev_syncs") for x, h in legs.items()},
           "handoff_failures": {x: h[0].engine.debug_get("handoff_failures") for x, h in legs.items()}}
    if len(names) == 2:
        num, den = ("rows", "torch") if metric == "rows" else ("graph", "eager")
        ratios = [a / b for a, b in zip(rows[num], rows[den])]
        out["ratio"] = "%s_over_%s" % (num, den)
        out["ratios"], out["ratio_median"] = ratios, float(np.median(ratios))
    if "graph" in legs:
        out["graph_captures"], out["graph_replays"] = legs["graph"][1].graph_captures, legs["graph"][1].graph_replays
    for h in legs.values():
        h[0].engine.close()
    return out


WRAP_NS = [64, 1024]
WRAP_COUNTERS = ("act_dev_calls", "step_rows_calls", "env_wrap_calls")


def _wrap_leg(leg, N, graph):
    """leg: "none" (the bare environment, its own limit 1000) | "torch" / "fused" (no limit of its own, the three wrappers on)"""
    import plugin
    from training.hip_tensor_env_wrappers import wrap_tensor_env

    kw = hip_kwargs(O, A, HID, B, seed=SEED, sample_batch_size=N, buffer_max_size=max(100_000, 4 * N), buffer_warm_size=max(B, N),
                    sample_interval=1, max_iteration=0, log_save_interval=10 ** 9, apprfunc_save_interval=10 ** 9,
                    eval_interval=10 ** 9, save_folder=None, ini_network_dir=None, strict_rng=False, hip_device_indices=True,
                    hip_pad_widths=True)
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    alg = plugin.create_alg(**kw)
    cls = SynthTensorHumanoid
    if graph:
        from synth_tensor_humanoid_inplace import SynthTensorHumanoidInplace as cls
    env = cls(N, device="cuda", seed=SEED, episode_limit=1000 if leg == "none" else 1 << 30)
    if leg != "none":
        env = wrap_tensor_env(env, max_episode_steps=1000, reward_shift=0.1, reward_scale=0.5,
                              obs_shift=np.linspace(-0.1, 0.1, O).astype(np.float32), obs_scale=np.linspace(0.5, 1.5, O).astype(np.float32))
        env.use_fused = leg == "fused"
    smp = plugin.create_sampler(**dict(kw, sampler_name="hip_tensor_env_sampler", env=env, **({"hip_graph_sample": True} if graph else {})))
    smp.networks = alg.networks
    return alg, smp, None


def run_wrap(N, names, graph, pairs, window):
    legs = {leg: _wrap_leg(leg, N, graph) for leg in names}
    counts, launches = {}, {}
    for leg, h in legs.items():                      # warm-up (eager call, capture, replays); its rate sizes the windows
        before = {k: h[0].engine.debug_get(k) for k in WRAP_COUNTERS}
        _window(*h, 1)                               # the first sample(): always issued eagerly, one lockstep step (S = N)
        launches[leg] = {k: h[0].engine.debug_get(k) - before[k] for k in WRAP_COUNTERS}
        dt = _window(*h, 4)
        dt = _window(*h, 4)
        counts[leg] = max(4, int(round(window / (dt / 4))))
    rows = {leg: [] for leg in legs}
    for _ in range(pairs):
        for leg, h in legs.items():
            dt = _window(*h, counts[leg])
            rows[leg].append(counts[leg] * N / dt)
    out = {"N": N, "graph": bool(graph), "unit": "env_steps_per_s", "window_counts": counts, "rows": rows,
           "median": {x: float(np.median(v)) for x, v in rows.items()},
           "spread": {x: (max(v) - min(v)) / float(np.median(v)) for x, v in rows.items()},
           "library_launches_per_lockstep_step": launches,
           "fused": {x: bool(getattr(h[1].env, "fused", False)) for x, h in legs.items()},
           "act_dev_syncs": {x: h[0].engine.debug_get("act_dev_syncs") for x, h in legs.items()},
           "handoff_failures": {x: h[0].engine.debug_get("handoff_failures") for x, h in legs.items()}}
    for num, den in (("fused", "torch"), ("fused", "none"), ("torch", "none")):
        if num in rows and den in rows:
            ratios = [a / b for a, b in zip(rows[num], rows[den])]
            out["%s_over_%s" % (num, den)] = {"ratios": ratios, "median": float(np.median(ratios))}
    if graph:
        out["graph_captures"] = {x: h[1].graph_captures for x, h in legs.items()}
        out["graph_replays"] = {x: h[1].graph_replays for x, h in legs.items()}
    for h in legs.values():
        h[0].engine.close()
    return out


def main_wrap(a):
    name = os.path.join(a.out, "env_wrap_bench.json")
    res = {"pairs": a.pairs, "window_s": a.window, "policy": "376-256-256-256-34", "max_episode_steps": 1000}
    if os.path.exists(name):                         # (the eager and the --graph run go into one file)
        with open(name) as f:
            res = json.load(f)
    key = "graph" if a.graph else "eager"
    res[key] = []
    for n in WRAP_NS:
        cmd = [sys.executable, os.path.abspath(__file__), "--wrap"] + a.wrap + ["--only", "%d:wrap" % n, "--pairs", str(a.pairs),
                                                                                "--window", str(a.window)] + (["--graph"] if a.graph else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("configuration %d:wrap failed (exit status %d)" % (n, p.returncode))
        r = json.loads(line[-1][len("RESULT "):])
        res[key].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(name, "w") as f:
        json.dump(res, f, indent=1)


def main_graph(a):
    parent = a.tree is not None
    name = os.path.join(a.out, "graph_sample_bench.json")
    res = {"pairs": a.pairs, "window_s": a.window, "policy": "376-256-256-256-34", "batch": B, "configs": [], "parent_eager": []}
    if os.path.exists(name):                         # (the two trees are run one after the other into one file)
        with open(name) as f:
            res = json.load(f)
    # (--tree pointing at this checkout: its own eager leg alone, the like-for-like partner of the other checkout's numbers)
    key = ("eager_alone" if ROOT == OUT_ROOT else "parent_eager") if parent else "configs"
    res[key] = []
    for n in GRAPH_NS:
        for metric in GRAPH_METRICS[:3] if parent else GRAPH_METRICS:
            cmd = [sys.executable, os.path.abspath(__file__), "--graph", "--only", "%d:%s" % (n, metric), "--pairs", str(a.pairs),
                   "--window", str(a.window)] + (["--tree", ROOT] if parent else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("configuration %d:%s failed (exit status %d)" % (n, metric, p.returncode))
            r = json.loads(line[-1][len("RESULT "):])
            res[key].append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(name, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(OUT_ROOT, "profiles"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.6)
    ap.add_argument("--only", default="", help="N:metric -- one configuration, in this process")
    ap.add_argument("--noise", action="store_true", help="only the tensor route's sampler rate without / with exploration noise")
    ap.add_argument("--noise-n", type=int, default=1024)
    ap.add_argument("--graph", action="store_true", help="only the tensor route eager against hip_graph_sample=True")
    ap.add_argument("--tree", default=None, help="with --graph: the eager leg alone from another checkout (the parent commit)")
    ap.add_argument("--wrap", nargs="+", choices=("none", "torch", "fused"), default=None,
                    help="only sample() alone with the reference's environment wrappers: the legs to run (with --graph: captured)")
    a = ap.parse_args()
    if a.wrap and a.only:
        print("RESULT " + json.dumps(run_wrap(int(a.only.split(":")[0]), a.wrap, a.graph, a.pairs, a.window)), flush=True)
        return
    if a.wrap:
        main_wrap(a)
        return
    if a.graph and a.only:
        n, metric = a.only.split(":")
        print("RESULT " + json.dumps(run_graph(int(n), metric, a.pairs, a.window, a.tree is not None)), flush=True)
        return
    if a.graph:
        main_graph(a)
        return
    if a.only:
        n, metric = a.only.split(":")
        print("RESULT " + json.dumps(run(int(n), metric, a.pairs, a.window)), flush=True)
        return
    res = {"pairs": a.pairs, "window_s": a.window, "policy": "376-256-256-256-34", "batch": B, "K": K, "configs": []}
    for n in [a.noise_n] if a.noise else NS:
        for metric in ("noise",) if a.noise else ("sampler", "trainer"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "%d:%s" % (n, metric), "--pairs", str(a.pairs),
                                "--window", str(a.window)], capture_output=True, text=True, timeout=420)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("configuration %d:%s failed (exit status %d)" % (n, metric, p.returncode))
            r = json.loads(line[-1][len("RESULT "):])
            res["configs"].append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "explore_noise_bench.json" if a.noise else "tensor_sampler_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
