"""fp32 vs coded image replay ring at the BASELINE.json configs[3] shape (DSAC_V2, CNN type_2, (3, 96, 96), B = 256), in one
process: two handles whose rings hold the same codebook-valued rows (default 100k rows: 22.1 GB fp32, 5.5 GB coded -- both
far larger than the 256 MB Infinity Cache), the same index table, and the same update sequence. CNN update steps/s are
taken as hipGraph replays (dsact_time_steps), alternating the two rings for --pairs pairs; the final parameters of the two
handles must be bitwise equal. Kernel times (k_gather_img vs k_gather_img_coded, the ring writers) come from running this
script under `rocprofv3 --kernel-trace --stats` with --trace (fewer steps, plus a few buffer adds), a separate run.

  python scripts/coded_ring_bench.py [--rows 100000] [--steps 400] [--warmup 50] [--pairs 3] [--trace] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -o coded -- python scripts/coded_ring_bench.py --trace
  python scripts/coded_ring_bench.py --summarize DIR/coded_results.db --out profiles/coded_ring_kernel_stats.csv   (no GPU)
"""
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

import bench  # noqa: E402  (make_cnn_alg: the configs[3] construction bench.py measures)

BOOK = np.float32(np.arange(256) / 255.0)


def fill_both(engines, n_rows, seed, chunk=1024):
    """the same codebook-valued rows into every ring (device-side generation, one chunk at a time)"""
    e0 = engines[0]
    g = torch.Generator(device=e0.device).manual_seed(seed)
    book = torch.as_tensor(BOOK, device=e0.device)
    O, A = e0.obs_dim, e0.act_dim
    for r0 in range(0, n_rows, chunk):
        n = min(chunk, n_rows - r0)
        obs = book.index_select(0, torch.randint(0, 256, (n * O,), device=e0.device, generator=g, dtype=torch.int32)).view(n, O)
        obs2 = book.index_select(0, torch.randint(0, 256, (n * O,), device=e0.device, generator=g, dtype=torch.int32)).view(n, O)
        act = torch.rand(n, A, device=e0.device, generator=g) * 2 - 1
        rew = torch.randn(n, device=e0.device, generator=g)
        done = (torch.rand(n, device=e0.device, generator=g) < 0.01).float()
        for e in engines:
            e.buffer_fill_device(r0, obs, act, rew, obs2, done)
    for e in engines:
        e.buffer_check()


def summarize(db, out):
    """the image gathers and ring writers of a --trace run's rocpd database, per kernel and grid: rows per launch (grid y)
    tells the fill (1024 rows) from the adds (8 rows)"""
    import sqlite3

    q = ("select name, grid_x, grid_y, grid_z, count(*), avg(duration), min(duration), max(duration) from kernels "
         "where name like '%gather_img%' or name like '%ring_write%' group by name, grid_x, grid_y, grid_z order by name, grid_y")
    lines = ["kernel,grid_x_workitems,grid_y,grid_z,calls,avg_us,min_us,max_us"]
    for name, gx, gy, gz, n, avg, lo, hi in sqlite3.connect(db).execute(q):
        lines.append('"%s",%d,%d,%d,%d,%.2f,%.2f,%.2f' % (name, gx, gy, gz, n, avg / 1e3, lo / 1e3, hi / 1e3))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--trace", action="store_true", help="short run for rocprofv3: 2 pairs of 40 steps, then 64 adds per ring")
    ap.add_argument("--out", default="")
    ap.add_argument("--summarize", default="", help="rocpd database of a --trace run: print (and write --out) the kernel table")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("coded_ring_bench: no GPU visible")
    if args.trace:
        args.steps, args.pairs, args.warmup = 40, 2, 8
    import __graft_entry__

    __graft_entry__.build()
    algs = {}
    for kind in ("fp32", "coded"):
        alg = bench.make_cnn_alg(0, seed=0, batch=args.batch)
        e = alg.engine
        e.buffer_create(args.rows, codebook=BOOK if kind == "coded" else None)
        algs[kind] = alg
    engines = [algs[k].engine for k in ("fp32", "coded")]
    t0 = time.time()
    fill_both(engines, args.rows, seed=100)
    fill_s = time.time() - t0
    for e in engines:
        bench.upload_indices(e, args.rows, 256, seed=1)
        e.set_device_rng(4242)
    gs = bench.graph_steps(args.steps, args.warmup)   # updates per captured graph: divides both step counts
    for e in engines:
        e.graph_build(gs)
        e.graph_run(0, args.warmup)
        e.sync()
    it = args.warmup
    pairs = []
    for p in range(args.pairs):
        order = ("fp32", "coded") if p % 2 == 0 else ("coded", "fp32")
        row = {}
        for kind in order:
            ms = algs[kind].engine.time_steps(it, args.steps, use_graph=True)
            row[kind] = args.steps / (ms / 1e3)
        it += args.steps
        row["coded_over_fp32"] = row["coded"] / row["fp32"]
        pairs.append(row)
    for e in engines:
        e.sync()
    same = all(torch.equal(getattr(engines[0], n), getattr(engines[1], n)) for n in ("online", "target", "adam_m", "adam_v"))
    same = same and engines[0].get_state() == engines[1].get_state()
    if args.trace:   # the ring writers: 64 adds of 8 transitions (the vectorised sampler's cadence) into each ring
        rng = np.random.default_rng(0)
        for _ in range(64):
            obs = BOOK[rng.integers(0, 256, (8, engines[0].obs_dim))]
            obs2 = BOOK[rng.integers(0, 256, (8, engines[0].obs_dim))]
            act = rng.uniform(-1, 1, (8, engines[0].act_dim)).astype(np.float32)
            rew, done = rng.standard_normal(8).astype(np.float32), np.zeros(8, np.float32)
            for e in engines:
                e.buffer_add(obs, act, rew, obs2, done)
        for e in engines:
            e.buffer_check()
    ratios = [r["coded_over_fp32"] for r in pairs]
    fp = [r["fp32"] for r in pairs]
    out = {
        "config": "configs[3]: DSAC_V2 CNN type_2 (3,96,96) B=%d, %d-row rings, codebook-valued rows, graph replays of %d steps"
                  % (args.batch, args.rows, args.steps),
        "buffer_bytes": {"fp32": engines[0].buffer_bytes, "coded": engines[1].buffer_bytes},
        "gather_ring_bytes_per_update": {"fp32": 2 * args.batch * engines[0].obs_dim * 4, "coded": 2 * args.batch * engines[0].obs_dim},
        "pairs": pairs,
        "coded_over_fp32": {"min": min(ratios), "median": float(np.median(ratios)), "max": max(ratios)},
        "fp32_spread": (max(fp) - min(fp)) / float(np.median(fp)),
        "bitwise_equal_state": bool(same),
        "fill_s": fill_s,
        "trace": bool(args.trace),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("coded_ring_bench: the coded ring's updates differ from the fp32 ring's")


if __name__ == "__main__":
    main()
