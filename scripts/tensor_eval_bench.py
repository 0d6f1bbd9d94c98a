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
Writes DIR/tensor_eval_bench.json and prints it. The library must have been built (__graft_entry__.build()).

  python scripts/tensor_eval_bench.py --graph [--out profiles] [--pairs 3]
      hip_graph_eval=True against the eager evaluator, both on tests/envs/synth_tensor_humanoid_inplace.py
      (the same dynamics with capture_safe = True), the same policy, E = N. Per N in 64, 256, 1024 (a fresh child process each):
      one warm-up evaluation per leg -- the captured leg's holds its eager window and its capture --, then `pairs` alternating
      (eager, graph) pairs of windows, the stream drained at each window's end. Medians, each leg's spread over its own windows,
      per-pair ratios (eager / graph) and the time per lockstep step are recorded. One more child: the captured leg at
      hip_eval_poll_steps P in 4, 16, 64, N = 256, the periods taken in turn inside each round.
      Writes DIR/graph_eval_bench.json. `--only eager:N` measures the eager leg of that comparison alone (it needs nothing this
      kwarg added: the figure to compare across two builds of the library).

  python scripts/tensor_eval_bench.py --save [--parent DIR] [--out profiles] [--pairs 3]
      eval_save=True against the evaluator without it, N = E = 256, a fresh child process per route: eager
      (tests/envs/synth_tensor_humanoid.py) and hip_graph_eval (its in-place twin). Legs, taken in turn inside each of `pairs`
      rounds: "off" (no kwarg), "save_1" (hip_eval_save_episodes=1: the extra launch per lockstep step, one file) and "save" (all
      256 episodes read back and written to a temporary folder, which is emptied between windows, outside the timing).
      --parent DIR: the one timing claim of the feature -- eval_save absent costs what it cost before. DIR is a built checkout of
      the commit to compare with; 2 * `pairs` pairs of fresh child processes, the order swapped from pair to pair, run
      `--only eager:256` from DIR and from this tree, and the ratio this / parent is recorded per pair with each side's spread.
      Writes DIR/tensor_eval_save_bench.json."""
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
from synth_tensor_humanoid_inplace import SynthTensorHumanoidInplace  # noqa: E402
from tensor_sampler_bench import OneEnv  # noqa: E402

NS = [64, 256, 1024]
PS = [1, 4, 16, 64]
GRAPH_PS = [4, 16, 64]
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


def _tensor(alg, N, P=None, graph=None, **more):
    """graph None: the section-16 leg (the plain fixture). False / True: the in-place fixture without / with hip_graph_eval"""
    import plugin

    kw = dict(more) if P is None else dict(more, hip_eval_poll_steps=P)
    if graph:
        kw["hip_graph_eval"] = True
    env = SynthTensorHumanoid if graph is None else SynthTensorHumanoidInplace
    return plugin.create_evaluator(evaluator_name="hip_tensor_env_evaluator", networks=alg.networks, num_eval_episode=N,
                                   eval_env=env(N, device="cuda", seed=SEED, episode_limit=LIMIT), **kw)


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


def run_graph(N, pairs, window, legs=("eager", "graph")):
    """the eager and the captured evaluator in alternating windows (legs = ("eager",): the eager leg alone)"""
    alg = _alg()
    evs = {leg: _tensor(alg, N, graph=leg == "graph") for leg in legs}
    reps, tars = {}, {}
    for leg, ev in evs.items():                       # warm-up (the captured leg: eager window + capture), then the sizing run
        tars[leg] = _window(alg, ev, 1)[1]
        reps[leg] = max(1, int(round(window / _window(alg, ev, 1)[0])))
    rows = {leg: [] for leg in evs}
    for _ in range(pairs):
        for leg, ev in evs.items():
            dt, tar = _window(alg, ev, reps[leg])
            rows[leg].append(dt)
            assert tar == tars[leg], (leg, tar, tars[leg])
    e = alg.engine
    steps = {leg: int(ev.steps) for leg, ev in evs.items()}
    out = {"N": N, "episodes": N, "metric": "seconds_per_run_evaluation", "repetitions_per_window": reps, "rows": rows,
           "lockstep_steps": steps, "tar": tars, "poll_steps": evs[legs[0]].poll_steps,
           "us_per_lockstep_step": {leg: 1e6 * float(np.median(v)) / steps[leg] for leg, v in rows.items()},
           "act_dev_syncs": e.debug_get("act_dev_syncs"), "handoff_failures": e.debug_get("handoff_failures")}
    if "graph" in evs:
        ratios = [a / g for a, g in zip(rows["eager"], rows["graph"])]
        out.update({"eager_over_graph": ratios, "eager_over_graph_median": float(np.median(ratios)),
                    "tar_bits_equal": np.float64(tars["eager"]).tobytes() == np.float64(tars["graph"]).tobytes(),
                    "graph_captures": evs["graph"].graph_captures, "graph_replays": evs["graph"].graph_replays})
    out.update(_stats(rows))
    e.close()
    return out


def run_graph_poll(N, pairs, window):
    """the captured leg at every poll period of GRAPH_PS (a window of the graph is P lockstep steps)"""
    alg = _alg()
    evs = {P: _tensor(alg, N, P, graph=True) for P in GRAPH_PS}
    reps = {}
    for P, ev in evs.items():
        _window(alg, ev, 1)
        reps[P] = max(1, int(round(window / _window(alg, ev, 1)[0])))
    rows = {P: [] for P in GRAPH_PS}
    for _ in range(pairs):
        for P, ev in evs.items():
            rows[P].append(_window(alg, ev, reps[P])[0])
    steps = {P: int(ev.steps) for P, ev in evs.items()}
    out = {"N": N, "episodes": N, "metric": "seconds_per_run_evaluation", "leg": "graph", "repetitions_per_window": reps,
           "rows": {str(P): v for P, v in rows.items()}, "lockstep_steps": {str(P): steps[P] for P in GRAPH_PS},
           "us_per_lockstep_step": {str(P): 1e6 * float(np.median(rows[P])) / steps[P] for P in GRAPH_PS},
           "graph_captures": {str(P): ev.graph_captures for P, ev in evs.items()}}
    out.update(_stats({str(P): v for P, v in rows.items()}))
    alg.engine.close()
    return out


def run_save(N, pairs, window, graph):
    """eval_save against the evaluator without it: legs off / save_1 / save in turn, `pairs` rounds"""
    import shutil
    import tempfile

    alg = _alg()
    root = tempfile.mkdtemp(prefix="tensor_eval_save_bench_")
    try:
        saved = {"off": 0, "save_1": 1, "save": N}
        evs = {leg: _tensor(alg, N, graph=True if graph else None,
                            **({} if not n else dict(eval_save=True, save_folder=os.path.join(root, leg), hip_eval_save_episodes=n,
                                                     hip_eval_save_max_steps=LIMIT)))
               for leg, n in saved.items()}

        def clean():
            alg.engine.sync()
            size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(root) for f in fs)
            for leg in saved:
                shutil.rmtree(os.path.join(root, leg), ignore_errors=True)
            return size

        reps, tars, written = {}, {}, {}
        for leg, ev in evs.items():                   # warm-up (the captured route: eager window + capture), then the sizing run
            tars[leg] = _window(alg, ev, 1)[1]
            clean()
            dt = _window(alg, ev, 1)[0]
            written[leg] = clean()                    # bytes one evaluation writes
            reps[leg] = max(1, int(round(window / dt))) if leg == "off" else 1
        rows = {leg: [] for leg in evs}
        for _ in range(pairs):
            for leg, ev in evs.items():
                dt, tar = _window(alg, ev, reps[leg])
                clean()
                rows[leg].append(dt)
                assert tar == tars[leg] == tars["off"], (leg, tar, tars)
        e = alg.engine
        steps = {leg: int(ev.steps) for leg, ev in evs.items()}
        out = {"route": "graph" if graph else "eager", "N": N, "episodes": N, "metric": "seconds_per_run_evaluation",
               "repetitions_per_window": reps, "rows": rows, "lockstep_steps": steps, "tar": tars, "poll_steps": evs["off"].poll_steps,
               "mean_episode_length": float(np.mean(evs["off"].lengths)), "bytes_written_per_evaluation": written,
               "trace_bytes": {leg: n * LIMIT * (4 * O + 4 * A + 4) for leg, n in saved.items()},
               "trace_dropped": {leg: int(ev.trace_dropped) for leg, ev in evs.items()},
               "us_per_lockstep_step": {leg: 1e6 * float(np.median(v)) / steps[leg] for leg, v in rows.items()},
               "over_off": {leg: [a / b for a, b in zip(rows[leg], rows["off"])] for leg in ("save_1", "save")},
               "eval_record_calls": e.debug_get("eval_record_calls"), "act_dev_syncs": e.debug_get("act_dev_syncs"),
               "handoff_failures": e.debug_get("handoff_failures")}
        if graph:
            out["graph_captures"] = {leg: ev.graph_captures for leg, ev in evs.items()}
        out.update(_stats(rows))
        e.close()
        return out
    finally:
        shutil.rmtree(root, ignore_errors=True)


def _child(script, only, pairs, window):
    cmd = ["timeout", "-k", "10", "300", sys.executable, script, "--only", only, "--pairs", str(pairs), "--window", str(window)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(script)))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit("configuration %s of %s failed (exit status %d)" % (only, script, p.returncode))
    return json.loads(line[-1][len("RESULT "):])


def save_main(a):
    res = {"pairs": a.pairs, "window_s": a.window, "policy": "376-256-256-256-34", "episode_limit": LIMIT, "N": 256, "configs": [],
           "off_against_parent": None}
    for only in ("save:256", "savegraph:256"):
        r = _child(os.path.abspath(__file__), only, a.pairs, a.window)
        res["configs"].append(r)
        print(json.dumps(r), flush=True)
    if a.parent:
        scripts = {"parent": os.path.join(os.path.abspath(a.parent), "scripts", "tensor_eval_bench.py"), "this": os.path.abspath(__file__)}
        rows = {k: [] for k in scripts}
        for i in range(2 * a.pairs):                  # pairs of fresh processes, the order swapped from pair to pair (a process that
            for k in (("parent", "this") if i % 2 == 0 else ("this", "parent")):     # follows another one starts on a warm device)
                rows[k].append(_child(scripts[k], "eager:256", a.pairs, a.window)["median"]["eager"])   # the child's median window
        ratios = [t / p for p, t in zip(rows["parent"], rows["this"])]
        res["off_against_parent"] = dict({"configuration": "eager:256 (no eval_save kwarg), seconds per run_evaluation, one fresh "
                                          "process per entry", "rows": rows, "this_over_parent": ratios,
                                          "this_over_parent_median": float(np.median(ratios))}, **_stats(rows))
        print(json.dumps(res["off_against_parent"]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "tensor_eval_save_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


def _one(only, pairs, window):
    if only.startswith("savegraph:"):
        return run_save(int(only[10:]), pairs, window, True)
    if only.startswith("save:"):
        return run_save(int(only[5:]), pairs, window, False)
    if only.startswith("graphpoll:"):
        return run_graph_poll(int(only[10:]), pairs, window)
    if only.startswith("graph:"):
        return run_graph(int(only[6:]), pairs, window)
    if only.startswith("eager:"):
        return run_graph(int(only[6:]), pairs, window, legs=("eager",))
    if only.startswith("poll:"):
        return run_poll(int(only[5:]), pairs, window)
    return run_n(int(only), pairs, window)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--only", default="", help="N, poll:N, graph:N, graphpoll:N or eager:N -- one configuration, in this process")
    ap.add_argument("--graph", action="store_true", help="hip_graph_eval against the eager evaluator -> graph_eval_bench.json")
    ap.add_argument("--save", action="store_true", help="eval_save against the evaluator without it -> tensor_eval_save_bench.json")
    ap.add_argument("--parent", default="", help="with --save: a built checkout of the commit to compare the kwarg-less evaluator with")
    a = ap.parse_args()
    if a.only:
        print("RESULT " + json.dumps(_one(a.only, a.pairs, a.window)), flush=True)
        return
    if a.save:
        return save_main(a)
    res = {"pairs": a.pairs, "window_s": a.window, "policy": "376-256-256-256-34", "episode_limit": LIMIT, "configs": [], "poll": None}
    todo = [str(n) for n in NS] + ["poll:256"]
    if a.graph:
        res["environment"] = "tests/envs/synth_tensor_humanoid_inplace.py"
        todo = ["graph:%d" % n for n in NS] + ["graphpoll:256"]
    for only in todo:
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--only", only, "--pairs", str(a.pairs),
               "--window", str(a.window)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("configuration %s failed (exit status %d)" % (only, p.returncode))
        r = json.loads(line[-1][len("RESULT "):])
        if only.startswith("poll:") or only.startswith("graphpoll:"):
            res["poll"] = r
        else:
            res["configs"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "graph_eval_bench.json" if a.graph else "tensor_eval_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
