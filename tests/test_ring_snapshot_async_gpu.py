"""Background ring snapshots on the GPU (dsact_buffer_shadow_take / _export / _digests / _release, k_ring_shadow,
HipReplayBuffer.save_async, HipOffSerialTrainer's hip_run_state_async). Every comparison is exact.

  1. the kernel: after a take every column of the shadow equals buffer_export and every chunk's six digests equal buffer_digest of
     that chunk -- chunks that start off 16-byte boundaries, one chunk, one row, a coded ring, a wrapped ring, and 70,000 one-row
     chunks (more than a grid dimension holds) against one vectorised NumPy restatement of the digest;
  2. isolation on the device: adds that wrap over the taken rows and a group of updates enqueued behind the take do not reach it;
  3. files: save_async's directory equals save()'s at the same ring state while adds continue; load() restores it;
  4. the trainer: background, synchronous and no snapshots end in the same state; run_state_24 equal; exact resume from the
     background run_state_24 -- device-resident pipeline (also wrapped by the save) and host pipeline;
  5. refusals (host-side checks: nothing here provokes a device fault), and the take does not wait."""
import json
import os
import pickle
import sys
import threading

import numpy as np
import pytest
import torch

from helpers import hip_kwargs
from test_ring_snapshot_gpu import (COLS, IMG, TABLE, _add, _assert_cols_equal, _assert_resumed_equals_straight, _buffer_on,
                                    _coded_engine, _coded_rows, _engine, _final_state, _rows, _scalars)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

FILES = [k + ".bin" for k in COLS] + ["meta.json"]


def _fill(e, rng, n, O, A, step=48):
    for r0 in range(0, n, step):
        _add(e, _rows(rng, min(step, n - r0), O, A))


def _check_shadow(e, chunk_rows):
    """take -> the shadow's rows and digests against the synchronous calls on the (unchanged) ring -> release"""
    size = e.buffer_size
    want = e.buffer_export(0, size)
    want_digs = [e.buffer_digest(r0, min(chunk_rows, size - r0)) for r0 in range(0, size, chunk_rows)]
    info = e.buffer_shadow_take(chunk_rows)
    assert (info["size"], info["ptr"], info["chunk_rows"], info["n_chunks"]) == (size, e.buffer_ptr, chunk_rows, len(want_digs))
    assert e.debug_get("shadow_state") == 1.0 and e.debug_get("shadow_bytes") >= info["bytes"] > 0
    _assert_cols_equal(e.buffer_shadow_export(0, size), want, chunk_rows)
    digs = e.buffer_shadow_digests()
    assert digs.shape == (len(want_digs), 6) and digs.dtype == np.uint64
    assert [tuple(int(v) for v in row) for row in digs] == want_digs, chunk_rows
    if size > 3:
        _assert_cols_equal(e.buffer_shadow_export(1, size - 3), {k: v[1:size - 2] for k, v in want.items()}, "sub-range")
    e.buffer_shadow_release()
    assert e.debug_get("shadow_state") == 0.0


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,A,rows,chunks", [(17, 6, 333, (7, 64, 1000)), (376, 17, 1, (64,)), (376, 17, 130, (64,))])
def test_shadow_equals_export_and_digest(O, A, rows, chunks):
    e = _engine(O, A, 400)
    _fill(e, np.random.default_rng(1), rows, O, A)
    assert e.buffer_size == rows
    takes = e.debug_get("shadow_takes")
    for chunk_rows in chunks:
        _check_shadow(e, chunk_rows)
    assert e.debug_get("shadow_takes") - takes == len(chunks)
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


def test_shadow_of_a_coded_ring():
    e, rng = _coded_engine(), np.random.default_rng(2)
    _add(e, _coded_rows(rng, 5))
    e.buffer_check()
    assert e.buffer_size == 5
    _check_shadow(e, 2)
    assert e.buffer_shadow_take(2)["n_chunks"] == 3 and e.buffer_shadow_export(0, 5)["obs"].dtype == np.uint8
    e.buffer_shadow_release(free=True)
    assert e.debug_get("shadow_bytes") == 0.0


def test_shadow_of_a_wrapped_and_of_an_empty_ring():
    O, A = 17, 6
    e = _engine(O, A, 200)
    info = e.buffer_shadow_take(64)                                  # empty: an empty shadow
    assert (info["size"], info["n_chunks"]) == (0, 0) and e.buffer_shadow_digests().shape == (0, 6)
    assert all(v.shape[0] == 0 for v in e.buffer_shadow_export(0, 0).values())
    e.buffer_shadow_release()
    _fill(e, np.random.default_rng(3), 288, O, A)                    # 288 transitions into 200 rows
    assert (e.buffer_size, e.buffer_ptr) == (200, 88)
    _check_shadow(e, 64)
    _check_shadow(e, 200)


def _numpy_digests_one_row_chunks(cols, widths):
    """section 18's digest of every ONE-ROW chunk, all rows at once: uint64 [rows, 6]"""
    u = np.uint64
    out = np.zeros((len(cols["rew"]), 6), np.uint64)
    with np.errstate(over="ignore"):
        for c, k in enumerate(COLS):
            w = widths[c]
            v = np.ascontiguousarray(cols[k]).reshape(-1).view(np.uint32).astype(np.uint64)
            x = np.arange(v.size, dtype=np.uint64) * u(0x9E3779B97F4A7C15) + ((u(c + 1) << u(32)) | v)
            x ^= x >> u(30)
            x *= u(0xBF58476D1CE4E5B9)
            x ^= x >> u(27)
            x *= u(0x94D049BB133111EB)
            x ^= x >> u(31)
            out[:, c] = x.reshape(-1, w).sum(axis=1, dtype=np.uint64)
    return out


def test_more_chunks_than_a_grid_dimension_holds():
    O, A, rows = 3, 1, 70000
    e = _engine(O, A, rows)
    r = _rows(np.random.default_rng(4), rows, O, A)
    _add(e, r)
    info = e.buffer_shadow_take(1)
    assert (info["size"], info["n_chunks"]) == (rows, rows)
    got = e.buffer_shadow_export(0, rows)
    _assert_cols_equal(got, r)
    digs = e.buffer_shadow_digests()
    want = _numpy_digests_one_row_chunks(r, (O, O, A, 1, 1, 1))
    assert digs.shape == want.shape == (rows, 6) and np.array_equal(digs, want)
    for k in (0, 65535, 65536, rows - 1):                            # ... and the restatement is section 18's digest
        assert tuple(int(v) for v in digs[k]) == e.buffer_digest(k, 1), k
    e.buffer_shadow_release()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def _learner(O=376, A=17, hid=(256, 256, 256), B=256, cap=1024, group=64, seed=1):
    from dsac_v2_hip import DSAC_V2_HIP

    torch.manual_seed(4)
    alg = DSAC_V2_HIP(**hip_kwargs(O, A, hid, B, seed=5, hip_pad_widths=True))
    e = alg.engine
    e.buffer_create(cap)
    _fill(e, np.random.default_rng(seed), cap, O, A, step=256)
    rows = np.random.default_rng(seed).integers(0, cap, size=(group, B))
    e.run_group(0, rows)                                             # (captures the group's graph: later calls are replays)
    e.sync()
    return alg, e, rows


def test_the_shadow_is_isolated_from_later_work():
    O, A, cap = 376, 17, 1024
    alg, e, rows = _learner(O, A, cap=cap)
    before = e.buffer_export(0, cap)
    before_digs = [e.buffer_digest(r0, min(300, cap - r0)) for r0 in range(0, cap, 300)]
    e.buffer_shadow_take(300)
    rng = np.random.default_rng(9)
    for _ in range(5):                                               # 1280 rows into 1024: every taken row is overwritten
        _add(e, _rows(rng, 256, O, A))
    e.run_group(64, rows)
    got = e.buffer_shadow_export(0, cap)
    digs = e.buffer_shadow_digests()
    _assert_cols_equal(got, before, "the rows of the moment of the take")
    assert [tuple(int(v) for v in row) for row in digs] == before_digs
    e.buffer_shadow_release()
    after = e.buffer_export(0, cap)
    assert not np.array_equal(after["act"], before["act"]) and e.buffer_ptr == 256
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_save_async_writes_what_save_writes(tmp_path):
    O, A, cap, B = 17, 6, 200, 64
    src = _engine(O, A, cap)
    _fill(src, np.random.default_rng(6), 288, O, A)                  # wrapped: size 200, ptr 88
    buf = _buffer_on(src, O, A, cap, B)
    buf.index_iteration = 11
    a = buf.save(tmp_path / "a", chunk_rows=64)
    reached, go = threading.Event(), threading.Event()

    def hold(i):
        if i == 0:
            reached.set()
            assert go.wait(60)

    job = buf.save_async(tmp_path / "b", chunk_rows=64, on_chunk=hold)
    assert reached.wait(60) and not job.done()
    rng = np.random.default_rng(7)
    for _ in range(5):                                               # adds continue while the writer is held
        _add(buf.engine, _rows(rng, 48, O, A))
    buf.index_iteration = 12
    go.set()
    job.wait()
    assert job.size == 200 and job.seconds > 0 and buf.snapshot_waits == 0 and buf.engine.debug_get("shadow_state") == 0.0
    assert sorted(os.listdir(a)) == sorted(os.listdir(job.path)) == sorted(FILES) and sorted(os.listdir(tmp_path)) == ["a", "b"]
    for k in COLS:
        assert open(os.path.join(a, k + ".bin"), "rb").read() == open(os.path.join(job.path, k + ".bin"), "rb").read(), k
    assert json.load(open(os.path.join(a, "meta.json"))) == json.load(open(os.path.join(job.path, "meta.json")))
    dst = _buffer_on(None, O, A, cap, B)
    dst.load(job.path)
    assert (dst.size, dst.ptr, dst.index_iteration) == (200, 88, 11)
    assert dst.engine.buffer_digest(0, 200) == src.buffer_digest(0, 200)
    assert buf.engine.buffer_digest(0, 200) != src.buffer_digest(0, 200)      # (the source ring itself moved on)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def _tensor_run(folder, cap, mode, resume=None):
    """section 18's device-resident case (tests/test_ring_snapshot_gpu.py): 48 iterations, a save at 24. mode: "bg", "sync", "none" """
    import plugin
    from synth_tensor_humanoid import SynthTensorHumanoid

    class Env(SynthTensorHumanoid):
        def state_dict(self):
            return {"pos": self.pos.cpu(), "t": self.t.cpu()}

        def load_state_dict(self, sd):
            self.pos, self.t = sd["pos"].to(self.device), sd["t"].to(self.device)

    O, A, N = 376, 17, 16
    kw = hip_kwargs(O, A, (64, 64), 64, buffer_max_size=cap, buffer_warm_size=128, seed=3, sample_batch_size=16, sample_interval=2,
                    max_iteration=48, log_save_interval=8, apprfunc_save_interval=24, eval_interval=16, num_eval_episode=4,
                    save_folder=folder, ini_network_dir=None, strict_rng=False, hip_device_indices=True, reward_scale=0.25,
                    sampler_name="hip_tensor_env_sampler", evaluator_name="hip_tensor_env_evaluator", hip_save_run_state=mode != "none",
                    hip_run_state_async=mode == "bg", hip_run_state_keep=4, ini_run_state_dir=resume, algorithm="DSAC_V2_HIP")
    torch.manual_seed(kw["seed"] if resume is None else 1234)
    np.random.seed(kw["seed"] if resume is None else 1234)
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    smp = plugin.create_sampler(env=Env(N, device="cuda", seed=4, episode_limit=torch.tensor([5, 1000] * (N // 2))), **kw)
    ev = plugin.create_evaluator(eval_env=SynthTensorHumanoid(4, device="cuda", seed=7, episode_limit=20), **kw)
    tr = plugin.create_trainer(alg, smp, buf, ev, **kw)
    if resume is not None:
        assert tr.iteration == 25 and buf.index_iteration == 25
    tr.train()
    assert tr._run_state_job is None and not [t for t in threading.enumerate() if t.name == "dsact-ring-snapshot"]
    assert alg.engine.debug_get("act_dev_syncs") == 0.0 and alg.engine.debug_get("handoff_failures") == 0.0
    return _final_state(alg, buf, smp), _scalars(folder)


def _host_run(folder, mode, resume=None):
    import plugin
    from synth_pendulum_data import SynthPendulum

    class Env(SynthPendulum):
        max_episode_steps = 30

        def state_dict(self):
            return {"rng": self.rng.bit_generator.state, "th": self.th, "thdot": self.thdot, "t": self.t}

        def load_state_dict(self, sd):
            self.rng.bit_generator.state = sd["rng"]
            self.th, self.thdot, self.t = sd["th"], sd["thdot"], sd["t"]

    class EvalEnv(SynthPendulum):
        max_episode_steps = 30

        def reset(self):
            self.rng = np.random.default_rng(11)
            return super().reset()

    kw = hip_kwargs(3, 1, (64, 64), 64, act_limit=2.0, buffer_max_size=512, buffer_warm_size=128, seed=3, sample_batch_size=16,
                    sample_interval=2, max_iteration=48, log_save_interval=8, apprfunc_save_interval=24, eval_interval=16,
                    num_eval_episode=2, save_folder=folder, ini_network_dir=None, strict_rng=False, reward_scale=0.25,
                    hip_save_run_state=mode != "none", hip_run_state_async=mode == "bg", hip_run_state_keep=4, ini_run_state_dir=resume)
    torch.manual_seed(kw["seed"] if resume is None else 1234)
    np.random.seed(kw["seed"] if resume is None else 1234)
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    smp = plugin.create_sampler(env=Env(seed=5), **kw)
    ev = plugin.create_evaluator(eval_env=EvalEnv(seed=6), **kw)
    tr = plugin.create_trainer(alg, smp, buf, ev, **kw)
    tr.train()
    assert tr._run_state_job is None and not [t for t in threading.enumerate() if t.name == "dsact-ring-snapshot"]
    st = _final_state(alg, buf, smp)
    st["rng"] = (np.random.get_state()[1].tobytes(), np.random.get_state()[2], torch.get_rng_state().numpy().tobytes())
    st["env"] = (smp.env.state_dict(), smp.obs.tobytes())
    return st, _scalars(folder)


def _same_run_state(a, b):
    """two run_state directories: ring files byte for byte, networks and optimiser by torch.equal, run.pkl as loaded dicts"""
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["networks.pkl", "optstate.pkl", "ring", "run.pkl"]
    assert sorted(os.listdir(os.path.join(a, "ring"))) == sorted(os.listdir(os.path.join(b, "ring"))) == sorted(FILES)
    for k in COLS:
        assert open(os.path.join(a, "ring", k + ".bin"), "rb").read() == open(os.path.join(b, "ring", k + ".bin"), "rb").read(), k
    assert json.load(open(os.path.join(a, "ring", "meta.json"))) == json.load(open(os.path.join(b, "ring", "meta.json")))

    def same(x, y, at):
        if isinstance(x, dict):
            assert isinstance(y, dict) and x.keys() == y.keys(), at
            for k in x:
                same(x[k], y[k], at + (k,))
        elif isinstance(x, (list, tuple)):
            assert type(x) is type(y) and len(x) == len(y), at
            for i, (p, q) in enumerate(zip(x, y)):
                same(p, q, at + (i,))
        elif torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()), at
        elif isinstance(x, np.ndarray):
            assert isinstance(y, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), at
        else:
            assert type(x) is type(y) and (x == y or (x != x and y != y)), (at, x, y)

    for fn in ("networks.pkl", "optstate.pkl"):
        same(torch.load(os.path.join(a, fn)), torch.load(os.path.join(b, fn)), (fn,))
    same(pickle.load(open(os.path.join(a, "run.pkl"), "rb")), pickle.load(open(os.path.join(b, "run.pkl"), "rb")), ("run.pkl",))


def _assert_same_end(a, b, sa, sb):
    for n in ("online", "target", "adam_m", "adam_v"):
        assert torch.equal(a[n], b[n]), n
    for n in ("state", "digest", "cursor", "sampler"):
        assert a[n] == b[n], (n, a[n], b[n])
    assert sa == sb and "Loss/Actor loss-RL iter" in sa               # every logged scalar but the wall-clock ones


@pytest.mark.parametrize("pipeline,cap", [("tensor", 512), ("tensor", 160), ("host", 512)])
def test_background_run_states_change_nothing_and_resume_exactly(tmp_path, pipeline, cap):
    run = (lambda f, m, resume=None: _tensor_run(f, cap, m, resume)) if pipeline == "tensor" else _host_run
    bg, s_bg = run(str(tmp_path / "bg"), "bg")
    sync, s_sync = run(str(tmp_path / "sync"), "sync")
    none, s_none = run(str(tmp_path / "none"), "none")
    _assert_same_end(bg, sync, s_bg, s_sync)
    _assert_same_end(bg, none, s_bg, s_none)
    d_bg, d_sync = (str(tmp_path / m / "apprfunc" / "run_state_24") for m in ("bg", "sync"))
    _same_run_state(d_bg, d_sync)
    _same_run_state(str(tmp_path / "bg" / "apprfunc" / "run_state_48"), str(tmp_path / "sync" / "apprfunc" / "run_state_48"))
    if pipeline == "tensor":
        meta = json.load(open(os.path.join(d_bg, "ring", "meta.json")))
        assert (meta["size"], meta["ptr"]) == (min(336, cap), 336 % cap) and meta["index_iteration"] == 25
    resumed, s_res = run(str(tmp_path / "resumed"), "bg", resume=d_bg)
    _assert_resumed_equals_straight(bg, resumed, s_bg, s_res)
    if pipeline == "host":
        assert bg["rng"] == sync["rng"] == none["rng"] == resumed["rng"] and bg["env"] == resumed["env"]


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    from dsact._ffi import DsactError
    from dsact.engine import DsactEngine

    O, A = 17, 6
    fresh = DsactEngine(O, A, [64, 64], 64)
    with pytest.raises(DsactError, match="E_STATE.*buffer not created"):
        fresh.buffer_shadow_take(64)
    e = _engine(O, A, 400)
    _fill(e, np.random.default_rng(5), 333, O, A)
    base = e.buffer_digest(0, 333)
    with pytest.raises(DsactError, match="E_STATE.*no shadow is taken"):
        e.buffer_shadow_export(0, 1)
    with pytest.raises(DsactError, match="E_STATE.*no shadow is taken"):
        e.buffer_shadow_digests()
    with pytest.raises(DsactError, match="E_INVALID.*chunk_rows"):
        e.buffer_shadow_take(0)
    need = e.buffer_shadow_take(64)["bytes"]
    e.buffer_shadow_release(free=True)
    takes = e.debug_get("shadow_takes")
    with pytest.raises(DsactError, match="E_INVALID.*max_bytes"):
        e.buffer_shadow_take(64, max_bytes=need - 1)                 # one byte too small: nothing allocated, nothing enqueued
    assert e.debug_get("shadow_state") == 0.0 and e.debug_get("shadow_bytes") == 0.0 and e.debug_get("shadow_takes") == takes
    assert e.stream_idle() and e.buffer_digest(0, 333) == base
    assert e.buffer_shadow_take(64, max_bytes=need)["bytes"] == need  # the exact bound passes
    with pytest.raises(DsactError, match="E_STATE.*not released"):
        e.buffer_shadow_take(64)
    for row0, n in ((0, 334), (300, 34), (-1, 2), (3, -1), (334, 0)):
        with pytest.raises(DsactError, match="E_INVALID.*rows taken"):
            e.buffer_shadow_export(row0, n)
    assert e.buffer_shadow_export(333, 0)["rew"].shape == (0,)
    e.buffer_shadow_release()
    # under stream capture: refused before anything is enqueued
    g = torch.cuda.CUDAGraph()
    refused = []
    with torch.cuda.graph(g, stream=e.torch_stream, capture_error_mode="relaxed"):
        try:
            e.buffer_shadow_take(64)
        except DsactError as ex:
            refused.append(str(ex))
    del g
    assert len(refused) == 1 and "E_STATE" in refused[0] and "under stream capture" in refused[0]
    assert e.debug_get("shadow_state") == 0.0 and e.debug_get("shadow_takes") == takes + 1
    assert e.buffer_digest(0, 333) == base
    e.buffer_shadow_take(64)                                         # the handle stays usable
    assert tuple(int(v) for v in e.buffer_shadow_digests().sum(axis=0, dtype=np.uint64)) == base
    e.buffer_shadow_release()
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


def test_the_take_does_not_wait():
    alg, e, rows = _learner()
    e.run_group(64, rows)                                            # 128 updates of the 3 x 256 Humanoid nets: milliseconds of work
    e.run_group(128, rows)
    info = e.buffer_shadow_take(300)
    busy = not e.stream_idle()
    assert busy, "dsact_buffer_shadow_take returned only after the stream had drained"
    want = e.buffer_export(0, info["size"])                          # (drains; the ring has not changed since the take)
    _assert_cols_equal(e.buffer_shadow_export(0, info["size"]), want)
    e.buffer_shadow_release()
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0
