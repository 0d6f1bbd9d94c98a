"""Ring snapshots and exact resume on the GPU (dsact_buffer_export / _import / _set_cursor / _digest, k_ring_digest,
HipReplayBuffer.save / load, HipOffSerialTrainer's hip_save_run_state / ini_run_state_dir):

  1. export == a NumPy restatement of the reference's store() after every wrapping add, logp included; sub-ranges, n = 0, refusals;
  2. import + set_cursor into a fresh engine: equal export, cursor, staged minibatch and later adds; unreachable cursors refused;
     outstanding minibatch tokens raise instead of training on the new rows;
  3. the coded ring: uint8 codes == np.searchsorted(table, value), bitwise round trip, a code >= n_codes refused;
  4. the digest kernel == ring_digest_reference on aligned and unaligned row slices, one row to several workgroups; additive;
     sees one bit and a row swap;
  5. save / load through files; a truncated file leaves the ring untouched, a corrupted one leaves it empty;
  6. - 8. a run resumed from run_state_24 ends bit for bit where the straight run ends: device-resident pipeline (also with a
     wrapped ring), host pipeline (strict_rng False / True), DSAC_V1.
Refusals are host-side argument checks: nothing here provokes a device fault."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
COLS = ("obs", "obs2", "act", "rew", "done", "logp")
WIDTHS = [(17, 6), (376, 17)]                       # 4-byte and 16-byte aligned ring rows
TABLE = np.float32(np.arange(200) / 255.0)          # 200 codes: a byte can name a missing entry
IMG = (3, 96, 96)


def _engine(O, A, cap, B=64):
    from dsact.engine import DsactEngine

    e = DsactEngine(O, A, [64, 64], B)
    e.buffer_create(cap)
    return e


def _rows(rng, n, O, A):
    f = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    return {"obs": f(n, O), "obs2": f(n, O), "act": f(n, A), "rew": f(n), "done": (rng.random(n) < 0.3).astype(np.float32), "logp": f(n)}


def _add(e, r):
    e.buffer_add(r["obs"], r["act"], r["rew"], r["obs2"], r["done"], r["logp"])


class _HostRing:
    """training/replay_buffer.py:58-79 restated: store() row by row with ptr = (ptr + 1) % N, size = min(size + 1, N)"""

    def __init__(self, cap, O, A):
        self.buf = {"obs": np.zeros((cap, O), np.float32), "obs2": np.zeros((cap, O), np.float32), "act": np.zeros((cap, A), np.float32),
                    "rew": np.zeros(cap, np.float32), "done": np.zeros(cap, np.float32), "logp": np.zeros(cap, np.float32)}
        self.ptr, self.size, self.cap = 0, 0, cap

    def store(self, r, i):
        for k in COLS:
            self.buf[k][self.ptr] = r[k][i]
        self.ptr = (self.ptr + 1) % self.cap
        self.size = min(self.size + 1, self.cap)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_cols_equal(got, want, what=""):
    for k in COLS:
        assert _same_bits(got[k], want[k]), (what, k)


def _filled(O, A, cap, adds, seed=0):
    """an engine after `adds` adds of 48 rows, and the host restatement of its ring"""
    e, ref, rng = _engine(O, A, cap), _HostRing(cap, O, A), np.random.default_rng(seed)
    for _ in range(adds):
        r = _rows(rng, 48, O, A)
        _add(e, r)
        for i in range(48):
            ref.store(r, i)
    return e, ref


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,A", WIDTHS)
def test_export_equals_the_reference_store(O, A):
    from dsact._ffi import DsactError

    cap = 200
    e, ref, rng = _engine(O, A, cap), _HostRing(cap, O, A), np.random.default_rng(1)
    assert e.buffer_export(0, 0)["obs"].shape == (0, O)              # an empty ring: n = 0 is a no-op
    for rnd in range(6):                                            # 288 transitions into 200 rows
        r = _rows(rng, 48, O, A)
        _add(e, r)
        for i in range(48):
            ref.store(r, i)
        assert (e.buffer_size, e.buffer_ptr) == (ref.size, ref.ptr)
        got = e.buffer_export(0, ref.size)
        _assert_cols_equal(got, {k: ref.buf[k][:ref.size] for k in COLS}, rnd)
        assert got["obs"].dtype == np.float32 and got["act"].shape == (ref.size, A) and got["logp"].shape == (ref.size,)
    _assert_cols_equal(e.buffer_export(7, 31), {k: ref.buf[k][7:38] for k in COLS}, "sub-range, odd row0")
    _assert_cols_equal(e.buffer_export(199, 1), {k: ref.buf[k][199:] for k in COLS}, "last row")
    assert all(v.shape[0] == 0 for v in e.buffer_export(200, 0).values())
    for row0, n in ((0, 201), (150, 51), (-1, 2), (3, -1), (201, 0)):
        with pytest.raises(DsactError, match="E_INVALID"):
            e.buffer_export(row0, n)
    _assert_cols_equal(e.buffer_export(0, 200), ref.buf, "the handle stays usable")
    fresh = _engine(O, A, cap)
    with pytest.raises(DsactError, match="E_INVALID"):
        fresh.buffer_export(0, 1)                                   # row0 + n <= size, not capacity


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,A", WIDTHS)
def test_import_and_cursor_rebuild_the_ring(O, A):
    from dsact._ffi import DsactError

    cap = 200
    a, ref = _filled(O, A, cap, 6)
    b = _engine(O, A, cap)
    epoch = b.fill_epoch
    whole = a.buffer_export(0, a.buffer_size)
    b.buffer_import(0, {k: v[:64] for k, v in whole.items()})       # in two parts, the second at an odd row
    b.buffer_import(64, {k: v[64:] for k, v in whole.items()})
    assert (b.buffer_size, b.buffer_ptr) == (0, 0) and b.fill_epoch > epoch   # an import moves neither size nor ptr
    b.buffer_set_cursor(a.buffer_size, a.buffer_ptr)
    assert (b.buffer_size, b.buffer_ptr) == (a.buffer_size, a.buffer_ptr) == (200, 88)
    _assert_cols_equal(b.buffer_export(0, 200), whole)
    idx = np.random.default_rng(2).integers(0, 200, 64)
    a.gather(idx)
    b.gather(idx)
    ba, bb = a.read_batch(with_logp=True), b.read_batch(with_logp=True)
    for k in COLS:
        assert _same_bits(ba[k], bb[k]), k
    more = _rows(np.random.default_rng(3), 48, O, A)
    _add(a, more)
    _add(b, more)
    assert (b.buffer_size, b.buffer_ptr) == (a.buffer_size, a.buffer_ptr) == (200, 136)
    _assert_cols_equal(b.buffer_export(0, 200), a.buffer_export(0, 200), "a further add lands on the same rows")
    assert _same_bits(a.buffer_export(88, 48)["act"], more["act"])
    # every pair the reference's store() cannot reach
    for size, ptr in ((-1, 0), (201, 0), (10, 9), (10, 11), (0, 1), (199, 0), (200, 200), (200, -1)):
        with pytest.raises(DsactError, match="E_INVALID"):
            b.buffer_set_cursor(size, ptr)
    assert (b.buffer_size, b.buffer_ptr) == (200, 136)
    with pytest.raises(DsactError, match="E_INVALID"):
        b.buffer_import(153, more)                                  # 153 + 48 > capacity
    with pytest.raises(ValueError):
        b.buffer_import(0, dict(more, obs=more["obs"].astype(np.float64)))
    _assert_cols_equal(b.buffer_export(0, 200), a.buffer_export(0, 200), "refused imports change nothing")
    for size, ptr in ((0, 0), (10, 10), (200, 0), (200, 199)):
        b.buffer_set_cursor(size, ptr)
        assert (b.buffer_size, b.buffer_ptr) == (size, ptr)


def test_outstanding_tokens_do_not_train_on_imported_rows():
    O, A, cap, B = 17, 6, 200, 64
    e, _ = _filled(O, A, cap, 6)
    buf = _buffer_on(e, O, A, cap, B)                              # a second handle holding a copy of the ring
    eng = buf.engine
    np.random.seed(0)
    staged = buf.sample_batch(B)                                    # still the staged minibatch when the import comes
    old = {k: staged[k].numpy().copy() for k in ("obs", "act", "logp")}
    stale = buf.sample_batch(B)
    later = buf.sample_batch(B)                                     # `stale` is no longer staged: it would have to re-gather
    group = buf.sample_batches(B, 2)
    new = _rows(np.random.default_rng(9), 200, O, A)
    eng.buffer_import(0, new)
    with pytest.raises(RuntimeError, match="overwritten"):
        stale.restage()
    with pytest.raises(RuntimeError, match="overwritten"):
        group.check_fresh()
    later.restage()                                                 # the staged copy was taken at sample time: the OLD rows
    got = eng.read_batch(with_logp=False)
    assert _same_bits(got["act"], e.buffer_export(0, 200)["act"][later.idxs])
    assert all(_same_bits(staged[k].numpy(), old[k]) for k in old)
    fresh = buf.sample_batch(B)
    assert _same_bits(fresh["act"].numpy(), new["act"][fresh.idxs])


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def _coded_engine(cap=48, B=16):
    from dsact.engine import DsactEngine
    from dsact.layout import CONV_TYPES

    e = DsactEngine(IMG, 3, CONV_TYPES["type_2"][4], B, conv_type="type_2")
    e.buffer_create(cap, codebook=TABLE)
    return e


def _coded_rows(rng, n):
    O = int(np.prod(IMG))
    r = _rows(rng, n, 1, 3)
    r["obs"], r["obs2"] = TABLE[rng.integers(0, len(TABLE), (n, O))], TABLE[rng.integers(0, len(TABLE), (n, O))]
    return r


@pytest.fixture(scope="module")
def coded_ring():
    """(engine, rows): a coded ring of 48 rows after 4 adds of 16 -- 64 transitions, wrapped -- and its host restatement"""
    e, rng = _coded_engine(), np.random.default_rng(4)
    ref = _HostRing(48, int(np.prod(IMG)), 3)
    for _ in range(4):
        r = _coded_rows(rng, 16)
        _add(e, r)
        for i in range(16):
            ref.store(r, i)
    e.buffer_check()
    return e, ref


def test_coded_ring_exports_codes_and_round_trips(coded_ring):
    from dsact._ffi import DsactError

    e, ref = coded_ring
    assert (e.buffer_size, e.buffer_ptr) == (48, 16)
    got = e.buffer_export(0, 48)
    for k in ("obs", "obs2"):
        assert got[k].dtype == np.uint8 and got[k].shape == (48, int(np.prod(IMG)))
        assert np.array_equal(got[k], np.searchsorted(TABLE, ref.buf[k]).astype(np.uint8)), k
    _assert_cols_equal({k: got[k] for k in COLS[2:]} | {"obs": got["obs"], "obs2": got["obs2"]},
                       {k: ref.buf[k] for k in COLS[2:]} | {"obs": got["obs"], "obs2": got["obs2"]})
    b = _coded_engine()
    b.buffer_import(0, got)
    b.buffer_set_cursor(48, 16)
    _assert_cols_equal(b.buffer_export(0, 48), got, "round trip")
    idx = np.arange(16) * 3
    e.gather(idx)
    b.gather(idx)
    ba, bb = e.read_batch(with_logp=True), b.read_batch(with_logp=True)
    for k in COLS:
        assert _same_bits(ba[k], bb[k]), k
    assert _same_bits(ba["obs"].reshape(16, -1), ref.buf["obs"][idx])    # the decoded values, bit for bit
    bad = {k: v[:5].copy() for k, v in got.items()}
    bad["obs2"][4, -1] = len(TABLE)                                  # the very last byte names no entry
    with pytest.raises(DsactError, match="E_INVALID.*code 200"):
        b.buffer_import(20, bad)
    _assert_cols_equal(b.buffer_export(0, 48), got, "a refused import leaves the ring unchanged")
    with pytest.raises(ValueError):
        b.buffer_import(0, dict(bad, obs=bad["obs"].astype(np.float32)))


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,A", WIDTHS)
def test_digest_kernel_equals_the_reference(O, A):
    from dsact._ffi import DsactError
    from dsact.engine import ring_digest_reference

    cap = 400
    e, ref = _filled(O, A, cap, 7, seed=5)                          # 336 live rows
    size = e.buffer_size
    assert size == 336
    w = (O, O, A, 1, 1, 1)
    whole = e.buffer_export(0, size)

    def want(row0, n):
        return ring_digest_reference({k: v[row0:row0 + n] for k, v in whole.items()}, row0, w)

    for row0, n in ((0, 1), (0, size), (3, 77), (size - 1, 1), (0, 333), (3, 333), (1, 2), (2, 5)):
        assert e.buffer_digest(row0, n) == want(row0, n), (row0, n)
    assert e.buffer_digest() == want(0, size) and e.buffer_digest(5) == want(5, size - 5)
    assert e.buffer_digest(17, 0) == (0,) * 6
    for cut in (1, 100, 335):                                       # additive over a split
        assert tuple((x + y) & M64 for x, y in zip(e.buffer_digest(0, cut), e.buffer_digest(cut, size - cut))) == want(0, size)
    for row0, n in ((0, size + 1), (size, 1), (-1, 1), (0, -1)):
        with pytest.raises(DsactError, match="E_INVALID"):
            e.buffer_digest(row0, n)
    base = e.buffer_digest(0, size)
    # one bit, written through buffer_import
    row = e.buffer_export(101, 1)
    row["act"].view(np.uint32)[0, A - 1] ^= 1
    e.buffer_import(101, row)
    whole = e.buffer_export(0, size)
    d = e.buffer_digest(0, size)
    assert [i for i in range(6) if d[i] != base[i]] == [2] and d == want(0, size)
    # two rows swapped: every column's digest moves (the index is the absolute ring row)
    r = next(i for i in range(100, size - 1) if whole["done"][i] != whole["done"][i + 1])   # (two rows that differ in every column)
    two = e.buffer_export(r, 2)
    e.buffer_import(r, {k: v[::-1].copy() for k, v in two.items()})
    whole = e.buffer_export(0, size)
    d2 = e.buffer_digest(0, size)
    assert all(d2[i] != d[i] for i in range(6)) and d2 == want(0, size)


def test_digest_kernel_on_the_coded_ring(coded_ring):
    from dsact.engine import ring_digest_reference

    e, _ = coded_ring
    O = int(np.prod(IMG))
    w = (O, O, 3, 1, 1, 1)
    whole = e.buffer_export(0, 48)
    for row0, n in ((0, 5), (0, 48), (7, 3)):
        assert e.buffer_digest(row0, n) == ring_digest_reference({k: v[row0:row0 + n] for k, v in whole.items()}, row0, w), (row0, n)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def _buffer_on(engine, O, A, cap, B, **over):
    """a HipReplayBuffer over a NEW handle of the engine's shape, with the engine's ring copied in"""
    from training.hip_replay_buffer import HipReplayBuffer

    if isinstance(O, tuple):
        from dsact.engine import DsactEngine
        from dsact.layout import CONV_TYPES
        eng = DsactEngine(O, A, CONV_TYPES["type_2"][4], B, conv_type="type_2")
    else:
        from dsact.engine import DsactEngine
        eng = DsactEngine(O, A, [64, 64], B)
    buf = HipReplayBuffer(obsv_dim=O, action_dim=A, buffer_max_size=cap, replay_batch_size=B, hip_engine=eng, **over)
    if engine is not None:
        eng.buffer_import(0, engine.buffer_export(0, engine.buffer_size))
        eng.buffer_set_cursor(engine.buffer_size, engine.buffer_ptr)
    return buf


@pytest.mark.parametrize("kind", ["fp32_17", "fp32_376", "coded"])
def test_save_and_load_through_files(tmp_path, kind, coded_ring):
    if kind == "coded":
        src_e, O, A, cap, B, over = coded_ring[0], IMG, 3, 48, 16, dict(hip_obs_codebook=TABLE)
    else:
        O, A = WIDTHS[0] if kind == "fp32_17" else WIDTHS[1]
        cap, B, over = 200, 64, {}
        src_e, _ = _filled(O, A, cap, 6, seed=6)                    # wrapped: size 200, ptr 88
    src = _buffer_on(src_e, O, A, cap, B, **over)
    src.index_iteration = 11
    path = src.save(tmp_path / "ring", chunk_rows=64)
    meta = json.load(open(os.path.join(path, "meta.json")))
    size = src.size
    assert (meta["size"], meta["ptr"], meta["capacity"]) == (size, src.ptr, cap) and len(meta["digests"]["chunks"]) == (size + 63) // 64
    assert [int(v, 16) for v in meta["digests"]["total"]] == list(src.engine.buffer_digest(0, size))
    want = src_e.buffer_export(0, size)
    dst = _buffer_on(None, O, A, cap, B, **over)
    dst.load(path)
    assert (dst.size, dst.ptr, dst.index_iteration) == (size, src.ptr, 11)
    _assert_cols_equal(dst.engine.buffer_export(0, size), want)
    assert dst.engine.buffer_digest(0, size) == src.engine.buffer_digest(0, size)
    # truncated: refused before anything touches the ring
    fn = os.path.join(path, "obs2.bin")
    data = open(fn, "rb").read()
    open(fn, "wb").write(data[:-1])
    with pytest.raises(ValueError, match="obs2.bin"):
        dst.load(path)
    assert (dst.size, dst.ptr) == (size, src.ptr)
    _assert_cols_equal(dst.engine.buffer_export(0, size), want, "untouched")
    # corrupted: the device's digest of the restored rows is not the saved one -- the ring is left empty
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 0x01
    open(fn, "wb").write(bytes(flipped))
    with pytest.raises(ValueError, match=r"chunk \d+ .*column obs2.*empty"):
        dst.load(path)
    assert (dst.size, dst.ptr) == (0, 0)


# ---- 6 - 8 ---------------------------------------------------------------------------------------------------------------------
TIME_TAGS = ("Time/", "Evaluation/2. TAR-Total time [s]")


def _scalars(folder):
    out = {}
    for line in open(os.path.join(folder, "scalars.jsonl")):
        r = json.loads(line)
        if not r["tag"].startswith(TIME_TAGS):
            out.setdefault(r["tag"], []).append((r["step"], r["value"]))
    return out


def _final_state(alg, buf, smp):
    e = alg.engine
    e.sync()
    st = {n: getattr(e, n).cpu().clone() for n in ("online", "target", "adam_m", "adam_v")}
    st["state"] = e.get_state()
    st["digest"] = e.buffer_digest(0, buf.size)
    st["cursor"] = (buf.size, buf.ptr, buf.index_iteration)
    st["sampler"] = (getattr(smp, "act_step", None), smp.get_total_sample_number())
    return st


def _assert_resumed_equals_straight(a, b, sa, sb, split=24):
    for n in ("online", "target", "adam_m", "adam_v"):
        assert torch.equal(a[n], b[n]), n
    for n in ("state", "digest", "cursor", "sampler"):
        assert a[n] == b[n], (n, a[n], b[n])
    assert set(sb) <= set(sa) and "Loss/Actor loss-RL iter" in sb and "Evaluation/1. TAR-RL iter" in sb
    for tag, rows in sb.items():
        assert rows and sa[tag][-len(rows):] == rows, tag           # every scalar of the resumed run, evaluation returns included
    for tag in ("Loss/Actor loss-RL iter", "Evaluation/1. TAR-RL iter", "RAM/RAM [MB]-RL iter"):
        assert [s for s, _ in sb[tag]] == [s for s, _ in sa[tag] if s > split], tag


def _tensor_run(folder, algorithm, cap, resume=None):
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
                    sampler_name="hip_tensor_env_sampler", evaluator_name="hip_tensor_env_evaluator", hip_save_run_state=True,
                    hip_run_state_keep=4, ini_run_state_dir=resume, algorithm=algorithm)
    if algorithm == "DSAC_V1_HIP":
        kw.update(TD_bound=10, bound=True)
    torch.manual_seed(kw["seed"] if resume is None else 1234)
    np.random.seed(kw["seed"] if resume is None else 1234)
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    smp = plugin.create_sampler(env=Env(N, device="cuda", seed=4, episode_limit=torch.tensor([5, 1000] * (N // 2))), **kw)
    ev = plugin.create_evaluator(eval_env=SynthTensorHumanoid(4, device="cuda", seed=7, episode_limit=20), **kw)
    tr = plugin.create_trainer(alg, smp, buf, ev, **kw)
    if resume is not None:
        assert tr.iteration == 25 and smp.get_total_sample_number() == 128 + 13 * 16 and buf.index_iteration == 25
    tr.train()
    return _final_state(alg, buf, smp), _scalars(folder)


@pytest.mark.parametrize("algorithm,cap", [("DSAC_V2_HIP", 512), ("DSAC_V2_HIP", 160), ("DSAC_V1_HIP", 512)])
def test_exact_resume_device_resident_pipeline(tmp_path, algorithm, cap):
    a, sa = _tensor_run(str(tmp_path / "a"), algorithm, cap)
    d = str(tmp_path / "a" / "apprfunc" / "run_state_24")
    meta = json.load(open(os.path.join(d, "ring", "meta.json")))
    assert (meta["size"], meta["ptr"]) == (min(336, cap), 336 % cap) and meta["index_iteration"] == 25
    b, sb = _tensor_run(str(tmp_path / "b"), algorithm, cap, resume=d)
    assert a["cursor"] == (min(512, cap), 512 % cap, 48) and a["sampler"] == (512 // 16, 512)
    _assert_resumed_equals_straight(a, b, sa, sb)


def _host_run(folder, strict, resume=None):
    import plugin
    from synth_pendulum_data import SynthPendulum

    class Env(SynthPendulum):
        max_episode_steps = 30

        def state_dict(self):
            return {"rng": self.rng.bit_generator.state, "th": self.th, "thdot": self.thdot, "t": self.t}

        def load_state_dict(self, sd):
            self.rng.bit_generator.state = sd["rng"]
            self.th, self.thdot, self.t = sd["th"], sd["thdot"], sd["t"]

    class EvalEnv(SynthPendulum):                                    # every evaluation starts from the same state: the evaluator
        max_episode_steps = 30                                       # carries none

        def reset(self):
            self.rng = np.random.default_rng(11)
            return super().reset()

    kw = hip_kwargs(3, 1, (64, 64), 64, act_limit=2.0, buffer_max_size=512, buffer_warm_size=128, seed=3, sample_batch_size=16,
                    sample_interval=2, max_iteration=48, log_save_interval=8, apprfunc_save_interval=24, eval_interval=16,
                    num_eval_episode=2, save_folder=folder, ini_network_dir=None, strict_rng=strict, reward_scale=0.25,
                    hip_save_run_state=True, hip_run_state_keep=4, ini_run_state_dir=resume)
    torch.manual_seed(kw["seed"] if resume is None else 1234)
    np.random.seed(kw["seed"] if resume is None else 1234)
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    smp = plugin.create_sampler(env=Env(seed=5), **kw)
    ev = plugin.create_evaluator(eval_env=EvalEnv(seed=6), **kw)
    tr = plugin.create_trainer(alg, smp, buf, ev, **kw)
    tr.train()
    st = _final_state(alg, buf, smp)
    st["rng"] = (np.random.get_state()[1].tobytes(), np.random.get_state()[2], torch.get_rng_state().numpy().tobytes())
    st["env"] = (smp.env.state_dict(), smp.obs.tobytes())
    return st, _scalars(folder)


@pytest.mark.parametrize("strict", [False, True])
def test_exact_resume_host_pipeline(tmp_path, strict):
    a, sa = _host_run(str(tmp_path / "a"), strict)
    b, sb = _host_run(str(tmp_path / "b"), strict, resume=str(tmp_path / "a" / "apprfunc" / "run_state_24"))
    _assert_resumed_equals_straight(a, b, sa, sb)
    assert a["rng"] == b["rng"]                                      # both generators end where the straight run's end
    assert a["env"] == b["env"]
