#!/usr/bin/env python3
"""Ring snapshots at scale: a 1M-row Humanoid fp32 ring (obs 376, act 17: 3.09 GB in HBM) --
seconds of HipReplayBuffer.save, of HipReplayBuffer.load, and of ONE whole-ring dsact_buffer_digest, the digest also as bytes/s
next to the HBM peak. Needs the GPU. None of these numbers is gated anywhere.

  python scripts/ring_snapshot_bench.py --leg save   --dir DIR [--rows 1000000] [--out profiles]
  python scripts/ring_snapshot_bench.py --leg load   --dir DIR      (reads what the save leg left in DIR)
  python scripts/ring_snapshot_bench.py --leg digest
One leg per process, so that a caller can put each under its own time limit; every leg merges its numbers into
OUT/ring_snapshot_bench.json and prints them. The save leg fills the ring with pseudo-random rows from device tensors
(dsact_buffer_fill_device), in slices; the snapshot in DIR is 3.09 GB on disk -- remove it afterwards."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dsac-v2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

O, A, B = 376, 17, 256
HBM_PEAK_MEASURED, HBM_PEAK_SPEC = 6.29e12, 8.0e12   # bytes/s: a float4 copy as measured on an MI355X, and the data-sheet figure


def _buffer(rows):
    from dsact.engine import DsactEngine
    from training.hip_replay_buffer import HipReplayBuffer

    eng = DsactEngine(O, A, [256, 256, 256], B)
    return HipReplayBuffer(obsv_dim=O, action_dim=A, buffer_max_size=rows, replay_batch_size=B, hip_engine=eng)


def _fill(buf, rows, slice_rows=65536):
    e = buf.engine
    g = torch.Generator(device="cuda").manual_seed(1)
    for r0 in range(0, rows, slice_rows):
        n = min(slice_rows, rows - r0)
        f = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
        e.buffer_fill_device(r0, f(n, O), f(n, A), f(n), f(n, O), (torch.rand(n, device="cuda", generator=g) < 0.01).float())
    e.sync()
    assert buf.size == rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["save", "load", "digest"])
    ap.add_argument("--dir", default=None)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--chunk-rows", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if args.leg in ("save", "load") and not args.dir:
        ap.error("--leg %s needs --dir" % args.leg)
    rows = args.rows
    ring_bytes = rows * 4 * (2 * O + A + 3)
    res = {"rows": rows, "obs_dim": O, "act_dim": A, "ring_bytes": ring_bytes, "chunk_rows": args.chunk_rows,
           "device": torch.cuda.get_device_name(0)}
    buf = _buffer(rows)
    e = buf.engine
    if args.leg == "save":
        _fill(buf, rows)
        t0 = time.perf_counter()
        buf.save(os.path.join(args.dir, "ring"), chunk_rows=args.chunk_rows, overwrite=True)
        res["save_seconds"] = time.perf_counter() - t0
        res["save_bytes_per_second"] = ring_bytes / res["save_seconds"]
    elif args.leg == "load":
        t0 = time.perf_counter()
        buf.load(os.path.join(args.dir, "ring"))
        res["load_seconds"] = time.perf_counter() - t0      # upload AND the digest check of every chunk
        res["load_bytes_per_second"] = ring_bytes / res["load_seconds"]
        assert buf.size == rows
    else:
        _fill(buf, rows)
        e.buffer_digest(0, rows)                              # (the first call allocates its six words)
        times = []
        for _ in range(5):
            t0 = time.perf_counter()
            d = e.buffer_digest(0, rows)
            times.append(time.perf_counter() - t0)
        part = [e.buffer_digest(r0, min(250000, rows - r0)) for r0 in range(0, rows, 250000)]
        assert tuple(sum(c) % (1 << 64) for c in zip(*part)) == d   # additive over a split, at this size too
        res["digest_seconds_each"] = times
        res["digest_seconds"] = sorted(times)[len(times) // 2]       # the median call, host clock around a synchronous call
        res["digest_bytes_per_second"] = ring_bytes / res["digest_seconds"]
        res["hbm_peak_bytes_per_second"] = {"measured_float4_copy": HBM_PEAK_MEASURED, "spec": HBM_PEAK_SPEC}
        res["digest_share_of_measured_peak"] = res["digest_bytes_per_second"] / HBM_PEAK_MEASURED
        res["digest"] = ["%016x" % v for v in d]
    os.makedirs(args.out, exist_ok=True)
    fn = os.path.join(args.out, "ring_snapshot_bench.json")
    merged = json.load(open(fn)) if os.path.exists(fn) else {}
    merged.update(res)
    with open(fn, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
