#!/usr/bin/env python3
"""HipOffAsyncTrainer against HipOffSerialTrainer on the CNN workload with the CNN acting path (hip_cnn_act=True; DESIGN.md
section 19): conv type_2 on the (3, 96, 96) image environment of tests/envs/synth_blob_data.py, batch 256, sample_interval 8,
sample_batch_size 8 -- the shape of the reference's example_train/dsacv2_cnn_carracing_offasync.py. Needs the GPU and a built
library.

  python scripts/cnn_async_bench.py [--out profiles] [--pairs 3]
      per configuration, in a fresh child process under its own time limit: one serial and one overlapped trainer, each with its
      own handle, then `pairs` timing windows of train() alternated between them, with the host time of the loop's phases (the
      sampler call among them). Configurations: HipOffSampler, and HipVecOffSampler with N = 8. A third child times one
      lockstep step of the vectorised sampler on its "gpu" route (dsact_act_sample_batch on the frames) against its "module"
      route (the stand-alone forward, a D2H copy of the logits, torch's Normal on the host) with the same weights.
      Nothing is started after a child that failed.
Writes DIR/cnn_async_bench.json and prints it."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dsac-v2_amd"), os.path.join(ROOT, "tests", "envs")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OBS, A, CONV, B, K = (3, 96, 96), 3, "type_2", 256, 8
CONFIGS = [
    dict(name="K8_single", N=0, iters=1600),
    dict(name="K8_vec8_gpu", N=8, iters=1600),
    dict(name="vec8_routes", N=8, routes=True, steps=400),
]
CHILD_LIMIT_S = 420


def kwargs(N=0, **over):
    kw = dict(
        env_id="synth_blob", algorithm="DSAC_V2_HIP", seed=7, action_type="continu", reward_scale=1, is_render=False,
        value_func_name="ActionValueDistri", value_func_type="CNN", value_conv_type=CONV, value_hidden_sizes=[256, 256, 256],
        value_hidden_activation="gelu", value_output_activation="linear", value_min_log_std=-8, value_max_log_std=8,
        policy_func_name="StochaPolicy", policy_func_type="CNN", policy_conv_type=CONV, policy_hidden_sizes=[256, 256, 256],
        policy_act_distribution="TanhGaussDistribution", policy_hidden_activation="gelu", policy_output_activation="linear",
        policy_min_log_std=-20, policy_max_log_std=0.5, value_learning_rate=1e-4, policy_learning_rate=1e-4,
        alpha_learning_rate=3e-4, gamma=0.99, tau=0.005, auto_alpha=True, alpha=0.2, delay_update=2, TD_bound=1, bound=True,
        trainer="off_serial_trainer", ini_network_dir=None, buffer_name="hip_replay_buffer", buffer_warm_size=512,
        buffer_max_size=4096, replay_batch_size=B, sample_interval=K, sample_batch_size=8, batch_size_per_sampler=8,
        noise_params=None, num_eval_episode=1, eval_interval=10 ** 9, eval_save=False, save_folder=None,
        apprfunc_save_interval=10 ** 9, log_save_interval=10 ** 9, max_iteration=10 ** 9, use_gpu=True, enable_cuda=True,
        obsv_dim=OBS, action_dim=A, action_high_limit=np.ones((A,), np.float32), action_low_limit=-np.ones((A,), np.float32),
        additional_info={}, cnn_shared=False, hip_device=0, hip_cnn_act=True,
    )
    if N:
        kw.update(sampler_name="hip_vec_off_sampler", vector_env_num=N)
    kw.update(over)
    return kw


def _trainer(cfg, trainer):
    import plugin

    kw = kwargs(cfg["N"], trainer=trainer)
    torch.manual_seed(kw["seed"])
    np.random.seed(kw["seed"])
    alg = plugin.create_alg(**kw)
    sampler = plugin.create_sampler(**kw)
    buf = plugin.create_buffer(**kw)
    tr = plugin.create_trainer(alg, sampler, buf, None, **dict(kw, max_iteration=0))
    if cfg["N"]:
        assert sampler.route() == "gpu", sampler.route()
    else:
        assert sampler.per_row_engine() is alg.engine
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
           "host_us_per_group": {k: {p: 1e6 * v * K / (pairs * cfg["iters"]) for p, v in ph.items()} for k, ph in phases.items()},
           "us_per_group": {k: [1e6 * K / r for r in v] for k, v in rows.items()},
           "us_per_group_median": {k: 1e6 * K / float(np.median(v)) for k, v in rows.items()}}
    for k in legs:
        out[k + "_median"] = float(np.median(rows[k]))
    out["async_over_serial"] = [a / s for a, s in zip(rows["async"], rows["serial"])]
    out["async_over_serial_median"] = float(np.median(out["async_over_serial"]))
    out["async_faster_in_every_pair"] = all(r > 1.0 for r in out["async_over_serial"])
    e = legs["async"][1].engine
    out["async_holds"] = e.debug_get("beh_holds")
    out["async_held_acts"] = e.debug_get("beh_acts")
    out["handoff_failures"] = {k: alg.engine.debug_get("handoff_failures") for k, (_, alg) in legs.items()}
    for _, alg in legs.values():
        alg.engine.close()
    return out


def run_routes(cfg, pairs):
    """one lockstep step of HipVecOffSampler (N frames -> N actions -> N environment steps) on the "gpu" route against the
    "module" route, on ONE handle's weights, alternated"""
    import plugin

    kw = kwargs(cfg["N"])
    torch.manual_seed(kw["seed"])
    alg = plugin.create_alg(**kw)
    smp = {"gpu": plugin.create_sampler(**kw), "module": plugin.create_sampler(**dict(kw, hip_cnn_act=False))}
    for s in smp.values():
        s.networks = alg.networks
    assert smp["gpu"].route() == "gpu" and smp["module"].route() == "module"
    steps_per_call = kw["sample_batch_size"] // cfg["N"]
    calls = cfg["steps"] // steps_per_call
    for s in smp.values():
        for _ in range(20):
            s.sample()
    rows = {k: [] for k in smp}
    for _ in range(pairs):
        for k, s in smp.items():
            alg.engine.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                s.sample()
            rows[k].append(1e6 * (time.perf_counter() - t0) / (calls * steps_per_call))
    # the environments' own share of a step (N resets-free steps of the image environment), for scale
    envs = smp["gpu"].envs
    act = np.zeros(A, np.float32)
    t0 = time.perf_counter()
    for _ in range(50):
        for e in envs:
            e.step(act)
    env_us = 1e6 * (time.perf_counter() - t0) / 50
    out = {"config": cfg, "us_per_lockstep_step": rows, "us_per_lockstep_step_median": {k: float(np.median(v)) for k, v in rows.items()},
           "env_steps_us_per_lockstep_step": env_us}
    out["module_over_gpu"] = [m / g for m, g in zip(rows["module"], rows["gpu"])]
    alg.engine.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--warm", type=int, default=160)
    ap.add_argument("--only", default="", help="one configuration name: run it in this process")
    a = ap.parse_args()
    from dsact import _ffi

    _ffi.load()   # (raises when the library has not been built: __graft_entry__.build())
    if a.only:
        cfg = next(c for c in CONFIGS if c["name"] == a.only)
        r = run_routes(cfg, a.pairs) if cfg.get("routes") else run_config(cfg, a.pairs, a.warm)
        print("RESULT " + json.dumps(r), flush=True)
        return
    res = {"shape": dict(obs=OBS, act_dim=A, conv_type=CONV, batch=B, sample_interval=K, sample_batch_size=8, env="synth_blob"),
           "pairs": a.pairs, "configs": []}
    for cfg in CONFIGS:
        # every child under its own time limit; a failure ends the run (nothing more is started on the GPU)
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--only", cfg["name"],
                            "--pairs", str(a.pairs), "--warm", str(a.warm)], capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit("configuration %s failed (exit status %d)" % (cfg["name"], p.returncode))
        r = json.loads(line[-1][len("RESULT "):])
        res["configs"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "cnn_async_bench.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
