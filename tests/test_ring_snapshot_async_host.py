"""Background ring snapshots on the CPU: HipReplayBuffer.save_async against a NumPy stand-in engine that
offers the four shadow calls, and the trainer's background run states with the stand-ins of tests/test_ring_snapshot_host.py.
Every comparison is exact. Nothing here needs a GPU; a writer thread is held with on_chunk and an Event, never with a sleep."""
import json
import os
import pickle
import re
import threading

import numpy as np
import pytest
import torch

from test_ring_snapshot_host import StandInEngine, TABLE, _cols, _fill, _parts

from dsact import _ffi
from dsact._ffi import DsactError
from dsact.engine import RING_COLUMNS, DsactEngine
from training.hip_replay_buffer import HipReplayBuffer, RingSaveJob

FILES = [k + ".bin" for k in RING_COLUMNS] + ["meta.json"]


class ShadowEngine(StandInEngine):
    """the stand-in with the four shadow calls: take copies the live rows and digests them, the readers serve that copy"""

    def __init__(self, *a):
        super().__init__(*a)
        self.shadow, self.takes, self.releases, self.freed = None, 0, 0, 0

    def buffer_shadow_take(self, chunk_rows, max_bytes=0):
        if self.shadow is not None:
            raise DsactError("E_STATE: a shadow has been taken and not released")
        if chunk_rows < 1:
            raise DsactError("E_INVALID: chunk_rows")
        size = self.buffer_size
        cols = {k: self.col[k][:size].copy() for k in RING_COLUMNS}
        nbytes = sum(v.nbytes for v in cols.values())
        if max_bytes and nbytes > max_bytes:
            raise DsactError("E_INVALID: max_bytes")
        digs = np.array([self.buffer_digest(r0, min(chunk_rows, size - r0)) for r0 in range(0, size, chunk_rows)],
                        dtype=np.uint64).reshape(-1, 6)
        self.shadow = (cols, digs)
        self.takes += 1
        return {"size": size, "ptr": self.buffer_ptr, "chunk_rows": chunk_rows, "n_chunks": len(digs), "bytes": nbytes}

    def buffer_shadow_export(self, row0, n):
        cols = self.shadow[0]
        assert 0 <= row0 and 0 <= n and row0 + n <= len(cols["rew"])
        return {k: cols[k][row0:row0 + n].copy() for k in RING_COLUMNS}

    def buffer_shadow_digests(self):
        return self.shadow[1].copy()

    def buffer_shadow_release(self, free=False):
        self.shadow = None
        self.releases += 1
        self.freed += bool(free)


def _buffer(O=5, A=3, cap=256, B=8, coded=False, **over):
    shape = (3, 4, 4) if coded else O
    eng = ShadowEngine(int(np.prod(shape)), A, B)
    kw = dict(obsv_dim=shape, action_dim=A, buffer_max_size=cap, replay_batch_size=B, hip_engine=eng)
    if coded:
        kw["hip_obs_codebook"] = TABLE
    kw.update(over)
    return HipReplayBuffer(**kw), eng


def _same_files(a, b):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == sorted(FILES)
    for fn in FILES:
        assert open(os.path.join(a, fn), "rb").read() == open(os.path.join(b, fn), "rb").read(), fn


class Gate:
    """an on_chunk that holds the writer after chunk `at` until open() -- the test thread waits for `reached` first"""

    def __init__(self, at=0):
        self.at, self.reached, self.go, self.seen = at, threading.Event(), threading.Event(), []

    def __call__(self, i):
        self.seen.append(i)
        if i == self.at:
            self.reached.set()
            assert self.go.wait(60)

    def open(self):
        self.go.set()


@pytest.mark.parametrize("case", ["ragged", "wrapped", "coded", "empty"])
def test_the_job_writes_what_save_writes(tmp_path, case):
    rng = np.random.default_rng(3)
    coded = case == "coded"
    cap = {"ragged": 256, "wrapped": 200, "coded": 48, "empty": 32}[case]
    size, ptr = {"ragged": (200, 200), "wrapped": (200, 77), "coded": (40, 40), "empty": (0, 0)}[case]
    buf, eng = _buffer(cap=cap, coded=coded)
    _fill(eng, rng, size, ptr, coded)
    buf.index_iteration = 31
    a = buf.save(tmp_path / "a", chunk_rows=64)
    seen = []
    job = buf.save_async(tmp_path / "b", chunk_rows=64, on_chunk=seen.append)
    assert isinstance(job, RingSaveJob) and job.path == str(tmp_path / "b") and job.size == size
    assert job.wait() == job.path and job.done() and job.seconds >= 0
    _same_files(a, job.path)
    assert seen == list(range((size + 63) // 64))                    # chunk by chunk: the host holds one chunk
    assert sorted(os.listdir(tmp_path)) == ["a", "b"] and eng.shadow is None and (eng.takes, eng.releases, eng.freed) == (1, 1, 0)
    other, eng2 = _buffer(cap=cap, coded=coded)
    other.load(job.path)                                             # load() needs no change
    assert (eng2.buffer_size, eng2.buffer_ptr, other.index_iteration) == (size, ptr, 31)
    assert eng2.buffer_digest(0, size) == eng.buffer_digest(0, size)


def test_the_files_are_those_of_the_moment_of_the_call(tmp_path):
    buf, eng = _buffer(cap=200)
    _fill(eng, np.random.default_rng(4), 200, 77)
    buf.index_iteration = 5
    a = buf.save(tmp_path / "a", chunk_rows=64)
    gate = Gate(0)
    job = buf.save_async(tmp_path / "b", chunk_rows=64, on_chunk=gate)
    assert gate.reached.wait(60) and not job.done()
    # the run goes on: rows are overwritten all over the ring, the cursor and the draw counter move
    new = _cols(np.random.default_rng(5), 150, 5, 3)
    eng.buffer_add(new["obs"], new["act"], new["rew"], new["obs2"], new["done"], new["logp"])
    buf.index_iteration = 99
    assert not os.path.exists(tmp_path / "b")                        # nothing appears before it is whole
    gate.open()
    job.wait()
    _same_files(a, job.path)
    meta = json.load(open(os.path.join(job.path, "meta.json")))
    assert (meta["size"], meta["ptr"], meta["index_iteration"]) == (200, 77, 5) and eng.buffer_ptr == (77 + 150) % 200


def test_refusals_come_first_on_the_calling_thread(tmp_path):
    buf, eng = _buffer()
    _fill(eng, np.random.default_rng(6), 100, 100)
    buf.save(tmp_path / "ring", chunk_rows=64)
    with pytest.raises(FileExistsError):
        buf.save_async(tmp_path / "ring", chunk_rows=64)
    with pytest.raises(ValueError, match="chunk_rows"):
        buf.save_async(tmp_path / "other", chunk_rows=0)
    assert eng.takes == 0 and buf._snapshot_job is None
    with pytest.raises(DsactError, match="max_bytes"):
        buf.save_async(tmp_path / "other", max_bytes=100)
    assert eng.shadow is None and buf._snapshot_job is None
    buf.save_async(tmp_path / "ring", chunk_rows=16, overwrite=True, keep_shadow=False).wait()
    assert json.load(open(tmp_path / "ring" / "meta.json"))["chunk_rows"] == 16 and eng.freed == 1
    assert sorted(os.listdir(tmp_path)) == ["ring"]

    buf2, _ = _buffer()
    buf2.engine = StandInEngine(5, 3, 8)                             # an engine without the shadow calls
    with pytest.raises(NotImplementedError, match="buffer_shadow_take"):
        buf2.save_async(tmp_path / "x")


def test_back_pressure_and_snapshot_waits(tmp_path):
    buf, eng = _buffer()
    _fill(eng, np.random.default_rng(7), 100, 100)
    gate = Gate(0)
    first = buf.save_async(tmp_path / "a", chunk_rows=64, on_chunk=gate)
    assert gate.reached.wait(60) and buf.snapshot_waits == 0
    threading.Timer(0.0, gate.open).start()                          # the second call below blocks until the first job ends
    eng.buffer_set_cursor(50, 50)
    second = buf.save_async(tmp_path / "b", chunk_rows=64)
    assert first.done() and buf.snapshot_waits == 1 and os.path.isdir(tmp_path / "a")
    second.wait()
    assert json.load(open(tmp_path / "a" / "meta.json"))["size"] == 100 and json.load(open(tmp_path / "b" / "meta.json"))["size"] == 50
    assert (eng.takes, eng.releases) == (2, 2)
    # save(), load() and dropping the buffer wait too
    for use in ("save", "load", "drop"):
        gate = Gate(0)
        job = buf.save_async(tmp_path / ("c_" + use), chunk_rows=64, on_chunk=gate)
        assert gate.reached.wait(60)
        threading.Timer(0.0, gate.open).start()
        if use == "save":
            buf.save(tmp_path / "d", chunk_rows=64)
        elif use == "load":
            buf.load(tmp_path / "a")
        else:
            buf.__del__()
        assert job.done() and eng.shadow is None and buf._snapshot_job is None and os.path.isdir(job.path)
    assert buf.snapshot_waits == 1                                   # (counts the save_async calls that waited)


def test_a_writer_failure_is_raised_by_wait_and_leaves_nothing(tmp_path):
    buf, eng = _buffer()
    _fill(eng, np.random.default_rng(8), 100, 100)
    (tmp_path / "file").write_bytes(b"x")
    job = buf.save_async(tmp_path / "file" / "ring", chunk_rows=64)    # the parent is a regular file
    with pytest.raises(OSError):
        job.wait()
    assert sorted(os.listdir(tmp_path)) == ["file"] and (tmp_path / "file").read_bytes() == b"x"
    assert eng.shadow is None and eng.releases == 1 and buf._snapshot_job is None

    def boom(i):
        raise RuntimeError("chunk %d" % i)

    job = buf.save_async(tmp_path / "ring", chunk_rows=64, on_chunk=boom)
    with pytest.raises(RuntimeError, match="chunk 0"):
        job.wait()
    assert sorted(os.listdir(tmp_path)) == ["file"] and eng.shadow is None      # the temporary directory is gone
    a = buf.save(tmp_path / "a", chunk_rows=64)
    _same_files(a, buf.save_async(tmp_path / "ring", chunk_rows=64).wait())     # the next one works


# ---- the trainer with stand-ins ------------------------------------------------------------------------------------------------------
def _async_parts(tmp_path, name, **over):
    kw, alg, smp, buf, ev = _parts(tmp_path, name, **over)
    buf = HipReplayBuffer(hip_engine=ShadowEngine(3, 1, 16), **kw)
    return kw, alg, smp, buf, ev


def _states(d):
    return sorted(fn for fn in os.listdir(d) if fn.startswith("run_state_"))


def test_background_run_states_complete_in_order_and_prune_late(tmp_path, monkeypatch):
    from training.hip_trainer import HipOffSerialTrainer

    kw, alg, smp, buf, ev = _async_parts(tmp_path, "a", hip_save_run_state=True, hip_run_state_async=True)
    tr = HipOffSerialTrainer(alg, smp, buf, ev, **kw)
    root = tmp_path / "a" / "apprfunc"
    order = []
    real_rename = os.rename
    monkeypatch.setattr(os, "rename", lambda a, b: (order.append((os.path.basename(b), sorted(os.listdir(os.path.dirname(b))))),
                                                   real_rename(a, b))[1])
    gates = {}
    real_save_async = buf.save_async

    def held(path, **k):                                             # every ring writer is held after its first chunk
        gates[path] = Gate(0)
        return real_save_async(path, on_chunk=gates[path], **k)

    buf.save_async = held
    for it in range(5):
        tr.iteration = it
        if it == 4:
            # the save point of iteration 4 joins the job of iteration 0 first: let it go from another thread
            threading.Timer(0.0, gates[str(root / "run_state_0" / "ring")].open).start()
        tr.step()
        if it == 0:
            g = gates[str(root / "run_state_0" / "ring")]
            assert g.reached.wait(60)
            assert sorted(os.listdir(root / "run_state_0")) == ["networks.pkl", "optstate.pkl"] + sorted(
                fn for fn in os.listdir(root / "run_state_0") if fn.startswith("ring.tmp-"))
    # run_state_0 completed before run_state_4 began: its ring directory first, its run.pkl last, with everything else there
    assert [o[0] for o in order[:2]] == ["ring", "run.pkl"] and order[1][1] == ["networks.pkl", "optstate.pkl", "ring", "run.pkl.tmp"]
    g4 = gates[str(root / "run_state_4" / "ring")]
    assert g4.reached.wait(60)
    # the writer of run_state_4 is held: the older complete directory is still there, the newer has no run.pkl yet
    assert _states(root) == ["run_state_0", "run_state_4"] and os.path.isfile(root / "run_state_0" / "run.pkl")
    assert os.path.isfile(root / "run_state_0" / "ring" / "meta.json") and not os.path.exists(root / "run_state_4" / "run.pkl")
    blob_before = pickle.load(open(root / "run_state_0" / "run.pkl", "rb"))
    assert blob_before["next_iteration"] == 1
    np.random.seed(12345)                                            # what the run does now must not leak into run.pkl
    g4.open()
    tr.wait_run_state()
    assert _states(root) == ["run_state_4"] and not [t for t in threading.enumerate() if t.name == "dsact-ring-snapshot"]
    assert sorted(os.listdir(root / "run_state_4")) == ["networks.pkl", "optstate.pkl", "ring", "run.pkl"]
    run = pickle.load(open(root / "run_state_4" / "run.pkl", "rb"))
    assert run["next_iteration"] == 5 and not np.array_equal(run["numpy_rng"][1], np.random.get_state()[1])
    assert json.load(open(root / "run_state_4" / "ring" / "meta.json"))["size"] == 150 == buf.size     # 100 + 5 x 20 rows into 150
    tr.wait_run_state()                                             # nothing pending: a no-op


def test_background_and_synchronous_run_states_are_equal_and_resume(tmp_path):
    from training.hip_trainer import HipOffSerialTrainer

    runs = {}
    for name, extra in (("sync", {}), ("bg", {"hip_run_state_async": True})):
        kw, alg, smp, buf, ev = _async_parts(tmp_path, name, hip_save_run_state=True, hip_run_state_keep=8, **extra)
        tr = HipOffSerialTrainer(alg, smp, buf, ev, **kw)
        tr.train()
        assert tr._run_state_job is None and buf._snapshot_job is None and buf.engine.shadow is None
        assert not [t for t in threading.enumerate() if t.name == "dsact-ring-snapshot"]
        runs[name] = tmp_path / name / "apprfunc"
    assert _states(runs["sync"]) == _states(runs["bg"]) == ["run_state_0", "run_state_12", "run_state_4", "run_state_8"]
    for st in _states(runs["sync"]):
        a, b = runs["sync"] / st, runs["bg"] / st
        assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["networks.pkl", "optstate.pkl", "ring", "run.pkl"]
        _same_files(a / "ring", b / "ring")
        ra, rb = pickle.load(open(a / "run.pkl", "rb")), pickle.load(open(b / "run.pkl", "rb"))
        assert ra.keys() == rb.keys() and ra["next_iteration"] == rb["next_iteration"] and ra["fingerprint"] == rb["fingerprint"]
        assert np.array_equal(ra["numpy_rng"][1], rb["numpy_rng"][1]) and torch.equal(ra["torch_rng"], rb["torch_rng"])
        assert ra["sampler"]["total_sample_number"] == rb["sampler"]["total_sample_number"]
        sa, sb = torch.load(a / "networks.pkl"), torch.load(b / "networks.pkl")
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
    # resume from a directory the background writer made
    d = str(runs["bg"] / "run_state_4")
    kw2, alg2, smp2, buf2, ev2 = _async_parts(tmp_path, "resumed", ini_run_state_dir=d)
    tr2 = HipOffSerialTrainer(alg2, smp2, buf2, ev2, **kw2)
    assert tr2.iteration == 5 and alg2.loaded["calls"] == 5
    tr2.train()
    assert alg2.calls == list(range(5, 12))


def test_a_train_that_raises_still_joins(tmp_path):
    from training.hip_trainer import HipOffSerialTrainer

    kw, alg, smp, buf, ev = _async_parts(tmp_path, "a", hip_save_run_state=True, hip_run_state_async=True)
    tr = HipOffSerialTrainer(alg, smp, buf, ev, **kw)
    real = alg.local_update

    def update(data, iteration):
        if iteration == 5:
            raise RuntimeError("update 5 failed")
        return real(data, iteration)

    alg.local_update = update
    with pytest.raises(RuntimeError, match="update 5 failed"):
        tr.train()
    root = tmp_path / "a" / "apprfunc"
    assert not [t for t in threading.enumerate() if t.name == "dsact-ring-snapshot"] and tr._run_state_job is None
    assert buf.engine.shadow is None
    # every directory with a run.pkl is whole (run_state_4 was in flight when the update raised)
    assert _states(root) == ["run_state_4"]
    assert sorted(os.listdir(root / "run_state_4")) == ["networks.pkl", "optstate.pkl", "ring", "run.pkl"]
    assert sorted(os.listdir(root / "run_state_4" / "ring")) == sorted(FILES)

    # a writer that fails: the next save point raises it, and nothing claims to be complete
    kw, alg, smp, buf, ev = _async_parts(tmp_path, "b", hip_save_run_state=True, hip_run_state_async=True)
    tr = HipOffSerialTrainer(alg, smp, buf, ev, **kw)
    buf.engine.buffer_shadow_export = lambda r0, n: (_ for _ in ()).throw(DsactError("E_HIP: the copy failed"))
    with pytest.raises(DsactError, match="the copy failed"):
        tr.train()
    rootb = tmp_path / "b" / "apprfunc"
    assert not [fn for st in _states(rootb) for fn in os.listdir(rootb / st) if fn == "run.pkl" or fn.startswith("ring")]
    assert not [t for t in threading.enumerate() if t.name == "dsact-ring-snapshot"]


def test_kwarg_refusals(tmp_path):
    from training.hip_async_trainer import HipOffAsyncTrainer
    from training.hip_trainer import HipOffSerialTrainer

    kw, alg, smp, buf, ev = _async_parts(tmp_path, "a", hip_run_state_async=True)
    with pytest.raises(ValueError, match="hip_save_run_state"):
        HipOffSerialTrainer(alg, smp, buf, ev, **kw)
    kw, alg, smp, _, ev = _async_parts(tmp_path, "b", hip_save_run_state=True, hip_run_state_async=True)

    class SyncOnly:
        size = 1000
        save = load = lambda self, *a, **k: None

    with pytest.raises(NotImplementedError, match="save_async"):
        HipOffSerialTrainer(alg, smp, SyncOnly(), ev, **kw)
    kw, alg, smp, buf, ev = _async_parts(tmp_path, "c", hip_save_run_state=True, hip_run_state_async=True)
    with pytest.raises(NotImplementedError, match="hip_save_run_state"):
        HipOffAsyncTrainer(alg, smp, buf, ev, **kw)
    kw, alg, smp, buf, ev = _async_parts(tmp_path, "d", hip_run_state_async=True)
    with pytest.raises(NotImplementedError, match="hip_run_state_async"):
        HipOffAsyncTrainer(alg, smp, buf, ev, **kw)

    class DataParallel:                                              # a handle that holds one shard of a larger batch
        class cfg:
            global_batch = 32
        batch, comm_world = 16, 1

    kw, alg, smp, buf, ev = _async_parts(tmp_path, "e", hip_save_run_state=True, hip_run_state_async=True)
    alg.engine = DataParallel()
    with pytest.raises(NotImplementedError, match="data-parallel"):
        HipOffSerialTrainer(alg, smp, buf, ev, **kw)
    # the two pass-through kwargs reach the buffer
    kw, alg, smp, buf, ev = _async_parts(tmp_path, "f", hip_save_run_state=True, hip_run_state_async=True,
                                         hip_snapshot_max_bytes=10, hip_snapshot_keep_shadow=False)
    tr = HipOffSerialTrainer(alg, smp, buf, ev, **kw)
    with pytest.raises(DsactError, match="max_bytes"):
        tr.step()
    kw["hip_snapshot_max_bytes"] = None
    kw, alg, smp, buf, ev = _async_parts(tmp_path, "g", hip_save_run_state=True, hip_run_state_async=True, hip_snapshot_keep_shadow=False)
    tr = HipOffSerialTrainer(alg, smp, buf, ev, **kw)
    tr.step()
    tr.wait_run_state()
    assert buf.engine.freed == 1


def test_the_five_symbols_are_declared_and_bound():
    names = {"dsact_buffer_shadow_take", "dsact_buffer_shadow_export", "dsact_buffer_shadow_digests", "dsact_buffer_shadow_release"}
    assert names | {"dsact_buffer_shadow_error"} <= {s[0] for s in _ffi.SYMBOLS}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsact.h")).read()
    for n in names:
        assert re.search(r"\bint %s\(dsact_handle\* h, " % n, header), n
    assert re.search(r"\bconst char\* dsact_buffer_shadow_error\(const dsact_handle\* h\);", header)
    assert "dsact_shadow_info" in header and [f[0] for f in _ffi.ShadowInfo._fields_] == ["size", "ptr", "chunk_rows", "n_chunks", "bytes"]
    for m in ("buffer_shadow_take", "buffer_shadow_export", "buffer_shadow_digests", "buffer_shadow_release"):
        assert callable(getattr(DsactEngine, m)), m
    assert callable(HipReplayBuffer.save_async)
