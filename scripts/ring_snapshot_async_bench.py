#!/usr/bin/env python3
"""Background ring snapshots at scale: a 1M-row Humanoid fp32 ring (obs 376, act 17: 3.09 GB in HBM).
Needs the GPU. None of these numbers is gated anywhere.

  python scripts/ring_snapshot_async_bench.py [--dir DIR] [--rows 1000000] [--rounds 3] [--iters 20000] [--save-every 5000]
  python scripts/ring_snapshot_async_bench.py --skip a,b --tag trainer_every_30000 --iters 90000 --save-every 30000 --rounds 1

The parent process touches no GPU: it starts every configuration as a fresh child under its own time limit, stops at the first
child that fails, and merges what the children print into OUT/ring_snapshot_async_bench.json.
  (a) scripts/ring_snapshot_bench.py --leg save / --leg load: wall time of the synchronous save() and load() (they also fill
      OUT/ring_snapshot_bench.json, section 18's measurement);
  (b) --child shadow: save_async -- seconds the calling thread is blocked (the first call allocates the shadow, the later ones
      do not), seconds until the snapshot is complete, and k_ring_shadow's device time between two events on the handle's
      stream; beside it, in the same process, the device time of the unfused alternative: six device-to-device copies of the
      columns' bytes plus one k_ring_digest per chunk;
  (c) --child train --mode none | sync | bg: HipOffSerialTrainer on the device-resident pipeline (hip_tensor_env_sampler, 256
      environments, sample_interval 8, hip_device_indices) over a full 1M-row ring, `--iters` iterations with a run state every
      `--save-every`: iterations / s and the seconds the training thread spent inside the save call. The three modes alternate,
      `--rounds` rounds; medians and each mode's spread over its rounds are recorded.
DIR receives 3.09 GB per snapshot (the trainer keeps one); it is removed afterwards."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dsac-v2_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "envs")):
    if p not in sys.path:
        sys.path.insert(0, p)

O, A, B, HID, N_ENVS, K, SEED = 376, 17, 256, (256, 256, 256), 256, 8, 3
CHILD_LIMIT = {"save": 300, "load": 300, "shadow": 300, "train": 420}     # seconds


def _fill(e, rows, slice_rows=65536):
    import torch

    g = torch.Generator(device="cuda").manual_seed(1)
    for r0 in range(0, rows, slice_rows):
        n = min(slice_rows, rows - r0)
        f = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
        e.buffer_fill_device(r0, f(n, O), f(n, A), f(n), f(n, O), (torch.rand(n, device="cuda", generator=g) < 0.01).float())
    e.sync()


def _median(v):
    s = sorted(v)
    return s[len(s) // 2]


def child_shadow(a):
    import torch

    from dsact.engine import DsactEngine
    from training.hip_replay_buffer import HipReplayBuffer

    rows, chunk = a.rows, a.chunk_rows
    eng = DsactEngine(O, A, list(HID), B)
    buf = HipReplayBuffer(obsv_dim=O, action_dim=A, buffer_max_size=rows, replay_batch_size=B, hip_engine=eng)
    _fill(eng, rows)
    assert buf.size == rows
    ring_bytes = rows * 4 * (2 * O + A + 3)
    res = {"rows": rows, "chunk_rows": chunk, "ring_bytes": ring_bytes, "device": torch.cuda.get_device_name(0)}
    stream = eng.torch_stream
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731

    # save_async: blocked / complete, three calls (the first allocates the shadow)
    blocked, complete = [], []
    for i in range(3):
        eng.sync()
        t0 = time.perf_counter()
        job = buf.save_async(os.path.join(a.dir, "shadow_ring"), chunk_rows=chunk, overwrite=True)
        t1 = time.perf_counter()
        job.wait()
        t2 = time.perf_counter()
        blocked.append(t1 - t0)
        complete.append(t2 - t0)
    res["save_async_blocked_seconds"] = blocked
    res["save_async_complete_seconds"] = complete
    res["writer_seconds_last"] = job.seconds

    # k_ring_shadow's device time (the digest memset and the launch, between two events on the handle's stream)
    fused = []
    for _ in range(5):
        eng.sync()
        e0, e1 = ev(), ev()
        e0.record(stream)
        eng.buffer_shadow_take(chunk)
        e1.record(stream)
        e1.synchronize()
        fused.append(e0.elapsed_time(e1) * 1e-3)
        eng.buffer_shadow_release()
    res["k_ring_shadow_device_seconds"] = fused
    res["k_ring_shadow_bytes_per_second"] = 2 * ring_bytes / _median(fused)      # read + written

    # the unfused alternative: six D2D copies of the columns' bytes, then one k_ring_digest per chunk
    widths = (O, O, A, 1, 1, 1)
    src = [torch.empty(rows * w, device="cuda") for w in widths]
    dst = [torch.empty(rows * w, device="cuda") for w in widths]
    copies, digests = [], []
    for _ in range(5):
        eng.sync()
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        with torch.cuda.stream(stream):
            e0.record(stream)
            for s, d in zip(src, dst):
                d.copy_(s)
            e1.record(stream)
        e1.synchronize()
        copies.append(e0.elapsed_time(e1) * 1e-3)
        total = 0.0
        for r0 in range(0, rows, chunk):
            e0, e1 = ev(), ev()
            e0.record(stream)
            eng.buffer_digest(r0, min(chunk, rows - r0))
            e1.record(stream)
            e1.synchronize()
            total += e0.elapsed_time(e1) * 1e-3
        digests.append(total)
    res["unfused_copy_device_seconds"] = copies
    res["unfused_digest_device_seconds"] = digests
    unfused = _median(copies) + _median(digests)
    res["unfused_device_seconds_median"] = unfused
    res["fused_device_seconds_median"] = _median(fused)
    res["fused_over_unfused"] = _median(fused) / unfused
    res["handoff_failures"] = eng.debug_get("handoff_failures")
    print("RESULT " + json.dumps(res, sort_keys=True))


def child_train(a):
    import numpy as np
    import torch

    import plugin
    from helpers import hip_kwargs
    from synth_tensor_humanoid import SynthTensorHumanoid

    class Env(SynthTensorHumanoid):
        def state_dict(self):
            return {"pos": self.pos.cpu(), "t": self.t.cpu()}

        def load_state_dict(self, sd):
            self.pos, self.t = sd["pos"].to(self.device), sd["t"].to(self.device)

    folder = os.path.join(a.dir, "train_" + a.mode)
    kw = hip_kwargs(O, A, HID, B, seed=SEED, sample_batch_size=N_ENVS, buffer_max_size=a.rows, buffer_warm_size=B, sample_interval=K,
                    max_iteration=a.iters, log_save_interval=10 ** 9, apprfunc_save_interval=a.save_every, eval_interval=10 ** 9,
                    save_folder=folder, ini_network_dir=None, strict_rng=False, hip_device_indices=True, hip_pad_widths=True,
                    sampler_name="hip_tensor_env_sampler", hip_save_run_state=a.mode != "none", hip_run_state_async=a.mode == "bg")
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    _fill(buf.engine, a.rows)                      # a full ring: every snapshot is the whole 3.09 GB
    assert buf.size == a.rows
    smp = plugin.create_sampler(env=Env(N_ENVS, device="cuda", seed=SEED), **kw)
    tr = plugin.create_trainer(alg, smp, buf, None, **kw)
    calls = []
    if a.mode != "none":
        inner = tr._save_run_state

        def timed(next_iteration):
            t0 = time.perf_counter()
            inner(next_iteration)
            calls.append(time.perf_counter() - t0)

        tr._save_run_state = timed
    alg.engine.sync()
    t0 = time.perf_counter()
    tr.train()
    alg.engine.sync()
    dt = time.perf_counter() - t0
    res = {"mode": a.mode, "iters": a.iters, "save_every": a.save_every, "seconds": dt, "iterations_per_s": a.iters / dt,
           "save_call_seconds": calls, "save_call_seconds_total": sum(calls), "snapshot_waits": getattr(buf, "snapshot_waits", 0),
           "handoff_failures": alg.engine.debug_get("handoff_failures"), "act_dev_syncs": alg.engine.debug_get("act_dev_syncs")}
    print("RESULT " + json.dumps(res, sort_keys=True))


def _child(args, limit):
    """one configuration in a fresh process under its own time limit; the object its RESULT line (or last line) holds"""
    print("[ring_snapshot_async_bench] %s" % " ".join(args[1:]), flush=True)
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit("child %r ended with status %d: nothing further is started" % (args[1:], r.returncode))
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    line = next((ln[len("RESULT "):] for ln in reversed(lines) if ln.startswith("RESULT ")), lines[-1])
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["shadow", "train"], default=None)
    ap.add_argument("--mode", choices=["none", "sync", "bg"], default="none")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--chunk-rows", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20000)
    ap.add_argument("--save-every", type=int, default=5000)
    ap.add_argument("--skip", default="", help="comma list of parts to leave out: a, b, c")
    ap.add_argument("--tag", default="trainer", help="key of part (c) in the JSON file (a second cadence beside the default one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.child == "shadow":
        return child_shadow(a)
    if a.child == "train":
        return child_train(a)
    own = a.dir is None
    a.dir = a.dir or tempfile.mkdtemp(prefix="ring_snapshot_async_bench-")
    os.makedirs(a.out, exist_ok=True)
    fn = os.path.join(a.out, "ring_snapshot_async_bench.json")
    res = json.load(open(fn)) if os.path.exists(fn) else {}
    res.update({"rows": a.rows, "obs_dim": O, "act_dim": A, "chunk_rows": a.chunk_rows})
    me = os.path.abspath(__file__)
    common = ["--dir", a.dir, "--rows", str(a.rows), "--chunk-rows", str(a.chunk_rows)]
    skip = set(a.skip.split(","))

    def keep():
        with open(fn, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)

    try:
        if "a" not in skip:
            sync_bench = os.path.join(os.path.dirname(me), "ring_snapshot_bench.py")
            s = _child([sync_bench, "--leg", "save", "--out", a.out] + common, CHILD_LIMIT["save"])
            ld = _child([sync_bench, "--leg", "load", "--out", a.out] + common, CHILD_LIMIT["load"])
            res["synchronous"] = {"save_seconds": s["save_seconds"], "load_seconds": ld["load_seconds"],
                                  "save_bytes_per_second": s["save_bytes_per_second"], "load_bytes_per_second": ld["load_bytes_per_second"]}
            shutil.rmtree(os.path.join(a.dir, "ring"), ignore_errors=True)
            keep()
        if "b" not in skip:
            res["shadow"] = _child([me, "--child", "shadow"] + common, CHILD_LIMIT["shadow"])
            shutil.rmtree(os.path.join(a.dir, "shadow_ring"), ignore_errors=True)
            keep()
        if "c" not in skip:
            rounds = []
            for _ in range(a.rounds):
                row = {}
                for mode in ("none", "sync", "bg"):
                    row[mode] = _child([me, "--child", "train", "--mode", mode, "--iters", str(a.iters), "--save-every", str(a.save_every)]
                                       + common, CHILD_LIMIT["train"])
                    shutil.rmtree(os.path.join(a.dir, "train_" + mode), ignore_errors=True)
                rounds.append(row)
                med = lambda m, k: _median([r[m][k] for r in rounds])   # noqa: E731
                spread = lambda m, k: (max(r[m][k] for r in rounds) - min(r[m][k] for r in rounds)) / med(m, k)   # noqa: E731
                res[a.tag] = {
                    "iters": a.iters, "save_every": a.save_every, "sample_interval": K, "n_envs": N_ENVS, "rounds": rounds,
                    "iterations_per_s_median": {m: med(m, "iterations_per_s") for m in ("none", "sync", "bg")},
                    "iterations_per_s_spread": {m: spread(m, "iterations_per_s") for m in ("none", "sync", "bg")},
                    "save_call_seconds_total_median": {m: med(m, "save_call_seconds_total") for m in ("sync", "bg")},
                    "bg_below_sync_in_every_round": all(r["bg"]["save_call_seconds_total"] < r["sync"]["save_call_seconds_total"] for r in rounds)}
                keep()
    finally:
        if own:
            shutil.rmtree(a.dir, ignore_errors=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
