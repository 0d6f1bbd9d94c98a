#!/usr/bin/env python3
"""The device-resident sampler on IMAGE environments (sampler_name="hip_tensor_env_sampler" with hip_cnn_act=True, DESIGN.md
section 20) against the best the vectorised sampler does for such an environment, on the SAME dynamics:
tests/envs/synth_tensor_blob.py (3 x 96 x 96, act 3). Policy and update are type_2 at batch 256. Needs the GPU.

  python scripts/tensor_image_sampler_bench.py [--out profiles] [--pairs 3] [--window 0.6]
      per N in 8, 64, 256 (each in a fresh child process under its own time limit) and per metric
        sampler: environment steps / s of sample() alone (one lockstep step per call, the stream drained at the window's end)
        trainer: iterations / s of HipOffSerialTrainer at sample_interval K = 8, hip_device_indices=True
      three legs, each with its own handle:
        vec  (a) HipVecOffSampler(hip_cnn_act=True) on its GPU route over N per-environment views (environment i alone on the
                 CPU device behind the gym-0.23 face), fp32 ring -- the baseline
        f32  (b) the tensor sampler on the batched environment with float32 frames, fp32 ring
        u8   (c) the tensor sampler with byte frames, coded ring
      one warm-up window per leg (which also sizes the windows to about --window seconds), then `pairs` alternating rounds of
      windows. Medians, per-round ratios (f32 / vec, u8 / vec, u8 / f32), each leg's spread over its own windows and the
      library's launches per sample() (acting chunks x launches per chunk + the ring write's; the environment's torch ops are
      not counted) are recorded.
Writes DIR/tensor_image_sampler_bench.json and prints it. The library must have been built (__graft_entry__.build()).

  python scripts/tensor_image_sampler_bench.py --graph [--out profiles] [--pairs 3] [--window 0.6]
      the opt-in of DESIGN.md section 24: the tensor sampler issued eagerly (tests/envs/synth_tensor_blob.py) against the same
      sampler with hip_graph_sample=True (sample() as one captured graph, on tests/envs/synth_tensor_blob_inplace.py), per N in
      64, 256, 1024, per frame dtype (u8: byte frames, coded ring; f32: float32 frames, fp32 ring) and per metric -- `sampler`
      (environment steps / s of sample() alone, one lockstep step per call) and `trainer1` / `trainer8` (iterations / s of
      HipOffSerialTrainer at sample_interval 1 / 8). Each configuration runs in a fresh child process under its own
      `timeout -k 10`; the first child that fails ends the run. One warm-up per leg (eager call, capture, replays), then `pairs`
      alternating rounds of an eager and a captured window, the stream drained at each window's end. Writes
      DIR/graph_image_bench.json; nothing else is run.

  python scripts/tensor_image_sampler_bench.py --pipe [--graph] [--out profiles] [--pairs 3] [--window 0.6]
      the reference's image pipeline of DESIGN.md section 28 (training/hip_tensor_frame_pipe.py): tests/envs/synth_tensor_rgb.py
      renders (3, 84, 84) uint8 RGB, hip_frame_pipe=True turns it into the (4, 84, 84) float32 gray stack with action_repeat 4
      for a type_1 policy. Two legs on twin handles: `torch` (the wrapper's torch route, use_fused = False) and `fused` (one
      launch behind every inner step and one behind the reset), per N in 64, 256, 1024, issued eagerly and with
      hip_graph_sample=True (--graph: the captured mode only). The metric is sample() alone, one lockstep step per call:
      OUTER environment steps / s and the host's microseconds per lockstep step. `frame_pipe_calls_per_step` is read from the
      debug counter: action_repeat + 1 on the fused leg, 0 on the torch leg. Each configuration runs in a fresh child process
      under its own `timeout -k 10`; the first child that fails ends the run. Writes DIR/frame_pipe_bench.json; nothing else is
      run."""
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

from synth_blob_data import _Box  # noqa: E402
from synth_tensor_blob import BOOK, SHAPE, SynthTensorBlob  # noqa: E402
from test_hip_cnn_parity import cnn_kwargs  # noqa: E402

NS = [8, 64, 256]
A, B, K, SEED, CAP = 3, 256, 8, 3, 4096
LEGS = ("vec", "f32", "u8")


class OneEnv:
    """environment i of the batched fixture on its own, with the interface HipVecOffSampler steps"""

    def __init__(self, i):
        self.env = SynthTensorBlob(1, seed=SEED, act_dim=A, env_offset=i)
        self.action_space = _Box(-np.ones(A), np.ones(A))
        self.observation_space = _Box(0.0, 1.0, shape=SHAPE)
        self.all = torch.ones(1, dtype=torch.bool)

    def reset(self):
        return self.env.reset(self.all)[0].numpy(), {}

    def step(self, a):
        o2, r, te, tr = self.env.step(torch.from_numpy(np.asarray(a, np.float32).reshape(1, A)))
        return o2[0].numpy(), float(r), bool(te), {"TimeLimit.truncated": bool(tr)}


def _leg(leg, N, trainer):
    import plugin

    kw = cnn_kwargs(SHAPE, A, "type_2", B, seed=SEED, sample_batch_size=N, buffer_max_size=CAP, buffer_warm_size=max(B, N),
                    sample_interval=K, max_iteration=0, log_save_interval=10 ** 9, apprfunc_save_interval=10 ** 9, eval_interval=10 ** 9,
                    save_folder=None, ini_network_dir=None, strict_rng=False, hip_device_indices=True, hip_cnn_act=True)
    if leg == "u8":
        kw["hip_obs_codebook"] = BOOK
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    alg = plugin.create_alg(**kw)
    if leg == "vec":
        smp = plugin.create_sampler(sampler_name="hip_vec_off_sampler", envs=[OneEnv(i) for i in range(N)], **kw)
    else:
        env = SynthTensorBlob(N, device="cuda", seed=SEED, act_dim=A, frames="uint8" if leg == "u8" else "float32")
        smp = plugin.create_sampler(sampler_name="hip_tensor_env_sampler", env=env, **kw)
    smp.networks = alg.networks
    buf = plugin.create_buffer(**kw)     # (always: byte frames are codes into the ring's codebook)
    tr = plugin.create_trainer(alg, smp, buf, None, **kw) if trainer else None
    if leg == "vec" and N > 1:
        assert smp.route() == "gpu", smp.route()
    return alg, smp, tr


def _window(alg, smp, tr, count):
    """`count` sample() calls, or `count` trainer iterations; seconds, the stream drained at both ends"""
    alg.engine.sync()
    t0 = time.perf_counter()
    if tr is None:
        for _ in range(count):
            smp.sample()
    else:
        tr.max_iteration = tr.iteration + count
        tr.train()
    alg.engine.sync()
    return time.perf_counter() - t0


def _library_launches(eng, smp, leg):
    """launches the library makes for one sample() + its ring write on a tensor leg: acting chunks x (ingest + conv layers +
    feature scatter + trunk layers + output) + the image columns' launch + the narrow columns' launch"""
    before = eng.debug_get("act_dev_calls")
    smp.sample()
    chunks = int(eng.debug_get("act_dev_calls") - before)
    per_chunk = 1 + len(eng.layout.geom) + 1 + len(eng.layout.hidden) + 1
    return {"acting_chunks": chunks, "launches_per_chunk": per_chunk, "ring_launches": 2, "total": chunks * per_chunk + 2}


GRAPH_NS = [64, 256, 1024]
GRAPH_METRICS = ("sampler", "trainer1", "trainer8")
GRAPH_FRAMES = ("u8", "f32")


def _graph_leg(leg, frames, N, k):
    """leg: "eager" (the plain tensor route) | "graph" (hip_graph_sample=True on the in-place fixture). frames: "u8" | "f32".
    k: sample_interval of a trainer, 0: sample() alone"""
    import plugin
    from synth_tensor_blob_inplace import SynthTensorBlobInplace

    kw = cnn_kwargs(SHAPE, A, "type_2", B, seed=SEED, sample_batch_size=N, buffer_max_size=max(CAP, 2 * N), buffer_warm_size=max(B, N),
                    sample_interval=max(k, 1), max_iteration=0, log_save_interval=10 ** 9, apprfunc_save_interval=10 ** 9,
                    eval_interval=10 ** 9, save_folder=None, ini_network_dir=None, strict_rng=False, hip_device_indices=True,
                    hip_cnn_act=True)
    if frames == "u8":
        kw["hip_obs_codebook"] = BOOK
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    alg = plugin.create_alg(**kw)
    cls, more = (SynthTensorBlob, {}) if leg == "eager" else (SynthTensorBlobInplace, {"hip_graph_sample": True})
    env = cls(N, device="cuda", seed=SEED, act_dim=A, frames="uint8" if frames == "u8" else "float32")
    smp = plugin.create_sampler(sampler_name="hip_tensor_env_sampler", env=env, **dict(kw, **more))
    smp.networks = alg.networks
    buf = plugin.create_buffer(**kw)     # (always: byte frames are codes into the ring's codebook)
    tr = plugin.create_trainer(alg, smp, buf, None, **kw) if k else None
    return alg, smp, tr


def run_graph(N, frames, metric, pairs, window):
    k = {"sampler": 0, "trainer1": 1, "trainer8": 8}[metric]
    legs = {leg: _graph_leg(leg, frames, N, k) for leg in ("eager", "graph")}
    unit = k or 1
    counts = {}
    for leg, h in legs.items():                      # warm-up (eager call, capture, replays); its rate sizes the windows
        c = 4 * unit
        dt = _window(*h, c)
        dt = _window(*h, c)
        counts[leg] = max(4 * unit, int(round(window / (dt / c) / unit)) * unit)
    rows = {leg: [] for leg in legs}
    for _ in range(pairs):
        for leg, h in legs.items():
            dt = _window(*h, counts[leg])
            rows[leg].append(counts[leg] * (N if not k else 1) / dt)
    ratios = [g / e for g, e in zip(rows["graph"], rows["eager"])]
    eng = legs["graph"][0].engine
    out = {"N": N, "frames": frames, "metric": metric, "unit": "iterations_per_s" if k else "env_steps_per_s", "window_counts": counts,
           "rows": rows, "median": {x: float(np.median(v)) for x, v in rows.items()},
           "spread": {x: (max(v) - min(v)) / float(np.median(v)) for x, v in rows.items()},
           "ratio": "graph_over_eager", "ratios": ratios, "ratio_median": float(np.median(ratios)),
           "graph_captures": legs["graph"][1].graph_captures, "graph_replays": legs["graph"][1].graph_replays,
           "launches_per_step": -(-N // 64) * (1 + len(eng.layout.geom) + 1 + len(eng.layout.hidden) + 1) + 1,
           "act_dev_syncs": {x: h[0].engine.debug_get("act_dev_syncs") for x, h in legs.items()},
           "handoff_failures": {x: h[0].engine.debug_get("handoff_failures") for x, h in legs.items()}}
    if not k:                                        # host time per lockstep step (= per sample() here), from the medians
        out["us_per_step"] = {x: 1e6 * N / out["median"][x] for x in rows}
    for h in legs.values():
        h[0].engine.close()
    return out


def main_graph(a):
    res = {"pairs": a.pairs, "window_s": a.window, "policy": "type_2 3x96x96, act 3", "batch": B, "ring_rows": CAP,
           "legs": {"eager": "HipTensorEnvSampler on SynthTensorBlob", "graph": "hip_graph_sample=True on SynthTensorBlobInplace"},
           "launches_per_step": "library launches of one lockstep step: acting chunks x (ingest + conv layers + feature scatter + "
                                "trunk layers + output) + the row move; the environment's torch ops are not counted",
           "configs": []}
    for n in GRAPH_NS:
        for frames in GRAPH_FRAMES:
            for metric in GRAPH_METRICS:
                what = "%d:%s:%s" % (n, frames, metric)
                # every GPU step under a time limit of its own; a child that fails ends the run: nothing more is started
                cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--graph", "--only", what,
                       "--pairs", str(a.pairs), "--window", str(a.window)]
                p = subprocess.run(cmd, capture_output=True, text=True)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit("configuration %s failed (exit status %d)" % (what, p.returncode))
                r = json.loads(line[-1][len("RESULT "):])
                res["configs"].append(r)
                print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "graph_image_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


PIPE_NS = [64, 256, 1024]
PIPE_SHAPE, PIPE_A, PIPE_K, PIPE_R = (4, 84, 84), 2, 4, 4


def _pipe_leg(leg, N, graph):
    """leg: "torch" | "fused" -- the same wrapped environment on either route of training/hip_tensor_frame_pipe.py"""
    import plugin
    from synth_tensor_rgb import SynthTensorRgb

    kw = cnn_kwargs(PIPE_SHAPE, PIPE_A, "type_1", B, seed=SEED, sample_batch_size=N, buffer_max_size=max(CAP, 2 * N),
                    buffer_warm_size=max(B, N), strict_rng=False, hip_cnn_act=True)
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    alg = plugin.create_alg(**kw)
    env = SynthTensorRgb(N, device="cuda", height=84, width=84, layout="chw", frames="uint8", act_dim=PIPE_A, act_limit=1.0)
    more = {"hip_graph_sample": True} if graph else {}
    smp = plugin.create_sampler(sampler_name="hip_tensor_env_sampler", env=env, hip_frame_pipe=True, frame_gray="chw",
                                frame_stack=PIPE_K, action_repeat=PIPE_R, **dict(kw, **more))
    smp.networks = alg.networks
    if leg == "torch":
        smp.env.use_fused = False
    return alg, smp, None


def run_pipe(N, mode, pairs, window):
    graph = mode == "graph"
    legs = {leg: _pipe_leg(leg, N, graph) for leg in ("torch", "fused")}
    counts, calls = {}, {}
    for leg, h in legs.items():                      # warm-up (eager call, capture, replays); its rate sizes the windows
        dt = _window(*h, 4)
        eng = h[0].engine
        before = eng.debug_get("frame_pipe_calls")
        dt = _window(*h, 4)
        # (a replayed graph makes no library call: the count is taken from the eager mode, where every launch is one)
        calls[leg] = None if graph else (eng.debug_get("frame_pipe_calls") - before) / 4.0
        counts[leg] = max(4, int(round(window / (dt / 4))))
    rows = {leg: [] for leg in legs}
    for _ in range(pairs):
        for leg, h in legs.items():
            dt = _window(*h, counts[leg])
            rows[leg].append(counts[leg] * N / dt)
    ratios = [f / t for f, t in zip(rows["fused"], rows["torch"])]
    out = {"N": N, "mode": mode, "unit": "outer_env_steps_per_s", "window_counts": counts, "rows": rows,
           "median": {x: float(np.median(v)) for x, v in rows.items()},
           "spread": {x: (max(v) - min(v)) / float(np.median(v)) for x, v in rows.items()},
           "us_per_step": {x: 1e6 * N / float(np.median(v)) for x, v in rows.items()},
           "ratio": "fused_over_torch", "ratios": ratios, "ratio_median": float(np.median(ratios)),
           "frame_pipe_calls_per_step": calls, "fused": {x: bool(h[1].env.fused) for x, h in legs.items()},
           "graph_replays": {x: h[1].graph_replays for x, h in legs.items()},
           "act_dev_syncs": {x: h[0].engine.debug_get("act_dev_syncs") for x, h in legs.items()},
           "handoff_failures": {x: h[0].engine.debug_get("handoff_failures") for x, h in legs.items()}}
    for h in legs.values():
        h[0].engine.close()
    return out


def main_pipe(a):
    res = {"pairs": a.pairs, "window_s": a.window, "policy": "type_1 4x84x84, act 2", "batch": B,
           "pipeline": "uint8 RGB (3, 84, 84) -> gray, frame_stack %d, action_repeat %d" % (PIPE_K, PIPE_R),
           "legs": {"torch": "FramePipeTensorEnv on its torch route", "fused": "one launch per inner step and one per reset"},
           "configs": []}
    for n in PIPE_NS:
        for mode in (("graph",) if a.graph else ("eager", "graph")):
            what = "%d:%s" % (n, mode)
            # every GPU step under a time limit of its own; a child that fails ends the run: nothing more is started
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--pipe", "--only", what,
                   "--pairs", str(a.pairs), "--window", str(a.window)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("configuration %s failed (exit status %d)" % (what, p.returncode))
            r = json.loads(line[-1][len("RESULT "):])
            res["configs"].append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "frame_pipe_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


def run(N, metric, pairs, window):
    trainer = metric == "trainer"
    unit = K if trainer else 1
    legs = {leg: _leg(leg, N, trainer) for leg in LEGS}
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
    ratio = lambda x, y: [p / q for p, q in zip(rows[x], rows[y])]
    ratios = {"f32_over_vec": ratio("f32", "vec"), "u8_over_vec": ratio("u8", "vec"), "u8_over_f32": ratio("u8", "f32")}
    out = {"N": N, "metric": "iterations_per_s" if trainer else "env_steps_per_s", "window_counts": counts, "rows": rows,
           "median": {k: float(np.median(v)) for k, v in rows.items()},
           "ratios": ratios, "ratio_medians": {k: float(np.median(v)) for k, v in ratios.items()},
           "spread": {k: (max(v) - min(v)) / float(np.median(v)) for k, v in rows.items()},
           "act_dev_syncs": {k: legs[k][0].engine.debug_get("act_dev_syncs") for k in ("f32", "u8")},
           "handoff_failures": {k: h[0].engine.debug_get("handoff_failures") for k, h in legs.items()}}
    if not trainer:
        out["library_launches_per_sample"] = {k: _library_launches(legs[k][0].engine, legs[k][1], k) for k in ("f32", "u8")}
    for h in legs.values():
        h[0].engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.6)
    ap.add_argument("--only", default="", help="N:metric -- one configuration, in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds a configuration's child process may take")
    ap.add_argument("--graph", action="store_true", help="only the tensor sampler eager against hip_graph_sample=True")
    ap.add_argument("--pipe", action="store_true", help="only the frame pipeline: its torch route against its fused route")
    a = ap.parse_args()
    if a.pipe and a.only:
        n, mode = a.only.split(":")
        print("RESULT " + json.dumps(run_pipe(int(n), mode, a.pairs, a.window)), flush=True)
        return
    if a.pipe:
        main_pipe(a)
        return
    if a.graph and a.only:
        n, frames, metric = a.only.split(":")
        print("RESULT " + json.dumps(run_graph(int(n), frames, metric, a.pairs, a.window)), flush=True)
        return
    if a.graph:
        main_graph(a)
        return
    if a.only:
        n, metric = a.only.split(":")
        print("RESULT " + json.dumps(run(int(n), metric, a.pairs, a.window)), flush=True)
        return
    res = {"pairs": a.pairs, "window_s": a.window, "policy": "type_2 3x96x96, act 3", "batch": B, "K": K, "ring_rows": CAP,
           "legs": {"vec": "HipVecOffSampler(hip_cnn_act=True), GPU route, N per-environment views, fp32 ring",
                    "f32": "HipTensorEnvSampler, float32 frames, fp32 ring", "u8": "HipTensorEnvSampler, uint8 frames, coded ring"},
           "configs": []}
    for n in NS:
        for metric in ("sampler", "trainer"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "%d:%s" % (n, metric), "--pairs", str(a.pairs),
                                "--window", str(a.window)], capture_output=True, text=True, timeout=a.limit)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("configuration %d:%s failed (exit status %d)" % (n, metric, p.returncode))
            r = json.loads(line[-1][len("RESULT "):])
            res["configs"].append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "tensor_image_sampler_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
