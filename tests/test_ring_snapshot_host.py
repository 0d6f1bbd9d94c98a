"""Ring snapshots and run states on the CPU: the digest's NumPy restatement against plain Python integers,
HipReplayBuffer.save / load against a NumPy stand-in engine that offers the four ring calls, and the trainer's run-state
directories with stand-ins in the style of tests/test_trainer_host.py. Nothing here needs a GPU."""
import json
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

from dsact import _ffi                                                     # noqa: E402
from dsact._ffi import DsactError                                          # noqa: E402
from dsact.engine import RING_COLUMNS, DsactEngine, ring_digest_reference  # noqa: E402
from training.hip_replay_buffer import RING_FORMAT, HipReplayBuffer        # noqa: E402

M64 = (1 << 64) - 1


# ---- the digest ----------------------------------------------------------------------------------------------------------------
def _mix(g, c, v):
    """include/dsact.h's definition, one element, in Python integers"""
    x = (g * 0x9E3779B97F4A7C15 + (((c + 1) << 32) | v)) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def _plain_digest(cols, row0, widths):
    out = []
    for c, k in enumerate(RING_COLUMNS):
        a = np.ascontiguousarray(cols[k])
        bits = a.reshape(-1).view(np.uint32) if a.dtype == np.float32 else a.reshape(-1)
        out.append(sum(_mix(row0 * widths[c] + i, c, int(v)) for i, v in enumerate(bits)) & M64)
    return tuple(out)


def _cols(rng, n, O, A, coded=False, n_codes=7):
    f = lambda *s: rng.standard_normal(s).astype(np.float32)       # noqa: E731
    img = (lambda: rng.integers(0, n_codes, (n, O)).astype(np.uint8)) if coded else (lambda: f(n, O))
    return {"obs": img(), "obs2": img(), "act": f(n, A), "rew": f(n), "done": (rng.random(n) < 0.3).astype(np.float32), "logp": f(n)}


@pytest.mark.parametrize("coded", [False, True])
def test_reference_equals_plain_python_integers(coded):
    rng = np.random.default_rng(0)
    O, A, n, row0 = 5, 3, 4, 7
    cols = _cols(rng, n, O, A, coded)
    cols["rew"][0] = np.float32(-0.0)                               # bits, not values: -0.0 is 0x80000000
    cols["act"][1, 2] = np.float32("nan")
    w = (O, O, A, 1, 1, 1)
    assert ring_digest_reference(cols, row0, w) == _plain_digest(cols, row0, w)
    assert ring_digest_reference(cols, row0) == _plain_digest(cols, row0, w)           # widths read off the arrays
    assert DsactEngine.ring_digest_reference(cols, row0, w) == _plain_digest(cols, row0, w)
    # an index past 2^32 elements stays a 64-bit integer: row 3e9 of a 5-wide column
    big = 3_000_000_000
    assert ring_digest_reference(cols, big, w) == _plain_digest(cols, big, w)
    assert ring_digest_reference({k: v[:0] for k, v in cols.items()}, 0, w) == (0,) * 6


def test_reference_is_additive_over_a_split():
    rng = np.random.default_rng(1)
    O, A, n, row0 = 17, 6, 50, 3
    cols = _cols(rng, n, O, A)
    w = (O, O, A, 1, 1, 1)
    whole = ring_digest_reference(cols, row0, w)
    for cut in (1, 19, 49):
        a = ring_digest_reference({k: v[:cut] for k, v in cols.items()}, row0, w)
        b = ring_digest_reference({k: v[cut:] for k, v in cols.items()}, row0 + cut, w)
        assert tuple((x + y) & M64 for x, y in zip(a, b)) == whole


def test_reference_sees_one_bit_and_a_row_swap():
    rng = np.random.default_rng(2)
    O, A, n = 9, 4, 12
    cols = _cols(rng, n, O, A)
    w = (O, O, A, 1, 1, 1)
    base = ring_digest_reference(cols, 0, w)
    for c, k in enumerate(RING_COLUMNS):
        flipped = {kk: v.copy() for kk, v in cols.items()}
        flipped[k].reshape(-1).view(np.uint32)[3] ^= 1              # the lowest mantissa bit of one element
        d = ring_digest_reference(flipped, 0, w)
        assert [i for i in range(6) if d[i] != base[i]] == [c]
    swapped = {k: v.copy() for k, v in cols.items()}
    for v in swapped.values():
        v[[2, 5]] = v[[5, 2]]
    d = ring_digest_reference(swapped, 0, w)
    assert all(d[i] != base[i] for i in range(6))                   # the index is the absolute ring row
    assert ring_digest_reference(cols, 1, w) != base


# ---- a NumPy engine with the four ring calls ---------------------------------------------------------------------------------------
class StandInEngine:
    """what HipReplayBuffer asks of an engine, in NumPy: the ring in stored form, the four snapshot calls with the library's
    refusals, and the add / gather bookkeeping the trainer stand-in test drives"""

    def __init__(self, O, A, B):
        self.obs_dim, self.act_dim, self.batch = O, A, B
        self.rows_added = self.fill_epoch = self.stage_serial = 0
        self.index_seed = 0
        self.imports = self.cursor_sets = 0

    def buffer_create(self, capacity, codebook=None):
        O, A, cap = self.obs_dim, self.act_dim, int(capacity)
        self.codebook = None if codebook is None else np.asarray(codebook, np.float32)
        odt = np.uint8 if codebook is not None else np.float32
        self.col = {"obs": np.zeros((cap, O), odt), "obs2": np.zeros((cap, O), odt), "act": np.zeros((cap, A), np.float32),
                    "rew": np.zeros(cap, np.float32), "done": np.zeros(cap, np.float32), "logp": np.zeros(cap, np.float32)}
        self.buffer_capacity, self.buffer_size, self.buffer_ptr = cap, 0, 0

    ring_widths = property(lambda self: (self.obs_dim, self.obs_dim, self.act_dim, 1, 1, 1))

    def set_index_rng(self, seed):
        self.index_seed = int(seed)

    def sync(self):
        pass

    def state(self):
        return (self.buffer_size, self.buffer_ptr, b"".join(self.col[k].tobytes() for k in RING_COLUMNS))

    def buffer_add(self, obs, act, rew, obs2, done, logp=None):
        assert self.codebook is None
        for i in range(len(rew)):
            p = self.buffer_ptr
            for k, v in (("obs", obs), ("obs2", obs2), ("act", act), ("rew", rew), ("done", done), ("logp", logp)):
                self.col[k][p] = v[i]
            self.buffer_ptr = (p + 1) % self.buffer_capacity
            self.buffer_size = min(self.buffer_size + 1, self.buffer_capacity)
        self.rows_added += len(rew)

    def gather(self, idx):
        self.stage_serial += 1

    def buffer_export(self, row0, n):
        if not (0 <= row0 and 0 <= n and row0 + n <= self.buffer_size):
            raise DsactError("E_INVALID: rows outside the live rows")
        return {k: self.col[k][row0:row0 + n].copy() for k in RING_COLUMNS}

    def buffer_import(self, row0, cols):
        n = len(cols["rew"])
        if not (0 <= row0 and row0 + n <= self.buffer_capacity):
            raise DsactError("E_INVALID: rows outside the capacity")
        for k in RING_COLUMNS:
            assert cols[k].dtype == self.col[k].dtype and cols[k].shape == self.col[k][row0:row0 + n].shape, k
        if self.codebook is not None and n and max(cols["obs"].max(), cols["obs2"].max()) >= len(self.codebook):
            raise DsactError("E_INVALID: a code is not below the codebook's entries")
        for k in RING_COLUMNS:
            self.col[k][row0:row0 + n] = cols[k]
        self.imports += 1
        self.fill_epoch += 1

    def buffer_set_cursor(self, size, ptr):
        cap = self.buffer_capacity
        if not (0 <= size <= cap and (ptr == size % cap if size < cap else 0 <= ptr < cap)):
            raise DsactError("E_INVALID: no state a ring reaches")
        self.buffer_size, self.buffer_ptr = size, ptr
        self.cursor_sets += 1

    def buffer_digest(self, row0=0, n=None):
        n = self.buffer_size - row0 if n is None else n
        return ring_digest_reference(self.buffer_export(row0, n), row0, self.ring_widths)


TABLE = np.float32(np.arange(7) / 7.0)


def _buffer(O=5, A=3, cap=256, B=8, coded=False, **over):
    shape = (3, 4, 4) if coded else O
    eng = StandInEngine(int(np.prod(shape)), A, B)
    kw = dict(obsv_dim=shape, action_dim=A, buffer_max_size=cap, replay_batch_size=B, hip_engine=eng)
    if coded:
        kw["hip_obs_codebook"] = TABLE
    kw.update(over)
    return HipReplayBuffer(**kw), eng


def _fill(eng, rng, size, ptr, coded=False):
    """the ring as `size` live rows with the cursor at `ptr` (rows written directly: the stand-in's own state)"""
    cols = _cols(rng, eng.buffer_capacity, eng.obs_dim, eng.act_dim, coded, n_codes=len(TABLE))
    for k in RING_COLUMNS:
        eng.col[k][:] = cols[k]
    eng.buffer_size, eng.buffer_ptr = size, ptr


@pytest.mark.parametrize("case", ["ragged", "wrapped", "coded", "empty"])
def test_save_load_round_trip(tmp_path, case):
    rng = np.random.default_rng(3)
    coded = case == "coded"
    cap = {"ragged": 256, "wrapped": 200, "coded": 48, "empty": 32}[case]
    size, ptr = {"ragged": (200, 200), "wrapped": (200, 77), "coded": (40, 40), "empty": (0, 0)}[case]
    buf, eng = _buffer(cap=cap, coded=coded)
    _fill(eng, rng, size, ptr, coded)
    buf.index_iteration = 31
    path = buf.save(tmp_path / "ring", chunk_rows=64)
    meta = json.load(open(os.path.join(path, "meta.json")))
    assert meta["format"] == RING_FORMAT == "dsact-ring-1" and (meta["capacity"], meta["size"], meta["ptr"]) == (cap, size, ptr)
    assert meta["chunk_rows"] == 64 and len(meta["digests"]["chunks"]) == (size + 63) // 64 and meta["index_iteration"] == 31
    assert meta["coded"] is coded and (meta["codebook"] == [int(b) for b in TABLE.view(np.uint32)] if coded else meta["codebook"] is None)
    assert [int(v, 16) for v in meta["digests"]["total"]] == list(eng.buffer_digest(0, size))
    for k in RING_COLUMNS:
        want = eng.col[k][:size]
        assert open(os.path.join(path, k + ".bin"), "rb").read() == want.astype(want.dtype.newbyteorder("<")).tobytes(), k
    assert sorted(os.listdir(tmp_path)) == ["ring"]                 # no temporary directory is left behind
    other, eng2 = _buffer(cap=cap, coded=coded)
    other.load(path)
    assert (eng2.buffer_size, eng2.buffer_ptr, other.index_iteration) == (size, ptr, 31)
    for k in RING_COLUMNS:
        assert np.array_equal(eng2.col[k][:size].view(np.uint8), eng.col[k][:size].view(np.uint8)), k
    assert eng2.imports == (size + 63) // 64                        # chunk by chunk: never more than chunk_rows rows on the host
    assert eng2.buffer_digest(0, size) == eng.buffer_digest(0, size)


def test_an_existing_target_needs_overwrite(tmp_path):
    buf, eng = _buffer()
    _fill(eng, np.random.default_rng(4), 100, 100)
    buf.save(tmp_path / "ring", chunk_rows=64)
    with pytest.raises(FileExistsError):
        buf.save(tmp_path / "ring", chunk_rows=64)
    eng.buffer_set_cursor(50, 50)
    buf.save(tmp_path / "ring", chunk_rows=16, overwrite=True)
    meta = json.load(open(tmp_path / "ring" / "meta.json"))
    assert meta["size"] == 50 and os.path.getsize(tmp_path / "ring" / "rew.bin") == 200
    assert sorted(os.listdir(tmp_path)) == ["ring"]


def _edit_meta(path, **kv):
    fn = os.path.join(path, "meta.json")
    meta = json.load(open(fn))
    meta.update(kv)
    json.dump(meta, open(fn, "w"))


REFUSALS = ["no_meta", "format", "capacity", "obs_shape", "act_dim", "coded", "codebook", "short_file", "long_file", "index_seed"]


@pytest.mark.parametrize("what", REFUSALS)
def test_every_refusal_leaves_the_ring_untouched(tmp_path, what):
    rng = np.random.default_rng(5)
    coded = what in ("codebook",)
    src, eng = _buffer(coded=coded, cap=64)
    _fill(eng, rng, 40, 40, coded)
    path = src.save(tmp_path / "ring", chunk_rows=16)
    over = {}
    if what == "no_meta":
        os.remove(os.path.join(path, "meta.json"))
    elif what == "format":
        _edit_meta(path, format="dsact-ring-0")
    elif what == "capacity":
        over = dict(cap=65)
    elif what == "obs_shape":
        over = dict(O=6)
    elif what == "act_dim":
        over = dict(A=4)
    elif what == "coded":
        _edit_meta(path, coded=True)
    elif what == "codebook":
        bits = [int(b) for b in TABLE.view(np.uint32)]
        bits[3] += 1                                                 # one entry, one bit
        _edit_meta(path, codebook=bits)
    elif what in ("short_file", "long_file"):
        fn = os.path.join(path, "act.bin")
        data = open(fn, "rb").read()
        open(fn, "wb").write(data[:-4] if what == "short_file" else data + b"\0\0\0\0")
    elif what == "index_seed":
        over = dict(hip_device_indices=True, hip_index_seed=99)      # the file was drawn with none: seed 0
    dst, eng2 = _buffer(coded=coded, **dict(dict(cap=64), **over))
    _fill(eng2, np.random.default_rng(6), 10, 10, coded)
    before = eng2.state()
    with pytest.raises(ValueError):
        dst.load(path)
    assert eng2.state() == before and eng2.imports == 0 and eng2.cursor_sets == 0


def test_a_flipped_byte_leaves_the_ring_empty_and_names_chunk_and_column(tmp_path):
    src, eng = _buffer()
    _fill(eng, np.random.default_rng(7), 200, 200)
    path = src.save(tmp_path / "ring", chunk_rows=64)
    fn = os.path.join(path, "act.bin")
    data = bytearray(open(fn, "rb").read())
    data[(64 * 2 + 5) * 3 * 4 + 1] ^= 0x10                           # row 133: chunk 2, column act
    open(fn, "wb").write(bytes(data))
    dst, eng2 = _buffer()
    with pytest.raises(ValueError) as ex:
        dst.load(path)
    assert re.search(r"chunk 2\b", str(ex.value)) and "column act" in str(ex.value) and "empty" in str(ex.value)
    assert (eng2.buffer_size, eng2.buffer_ptr) == (0, 0)


def test_the_four_symbols_are_declared_and_bound():
    names = {"dsact_buffer_export", "dsact_buffer_import", "dsact_buffer_set_cursor", "dsact_buffer_digest"}
    assert names <= {s[0] for s in _ffi.SYMBOLS}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dsact.h")).read()
    for n in names:
        assert re.search(r"\bint %s\(dsact_handle\* h, " % n, header), n
    for m in ("buffer_export", "buffer_import", "buffer_set_cursor", "buffer_digest", "ring_digest_reference"):
        assert callable(getattr(DsactEngine, m)), m


# ---- samplers and the trainer with stand-ins --------------------------------------------------------------------------------------
def _pendulum(seed=3, with_state=True):
    from synth_pendulum_data import SynthPendulum

    class Env(SynthPendulum):
        def state_dict(self):
            return {"rng": self.rng.bit_generator.state, "th": self.th, "thdot": self.thdot, "t": self.t}

        def load_state_dict(self, sd):
            self.rng.bit_generator.state = sd["rng"]
            self.th, self.thdot, self.t = sd["th"], sd["thdot"], sd["t"]

    return (Env if with_state else SynthPendulum)(seed=seed)


class StubAlg:
    def __init__(self, networks):
        self.networks = networks
        self.calls, self.loaded = [], None

    def local_update(self, data, iteration):
        self.calls.append(iteration)
        return {"Loss/Critic loss-RL iter": 1.0 / (1 + iteration), "Time/Algorithm time [ms]-RL iter": 0.1}

    def optimizer_state_dict(self):
        return {"format": "stub", "calls": len(self.calls)}

    def load_optimizer_state_dict(self, sd):
        self.loaded = sd


def _parts(tmp_path, name, env=None, **over):
    from dsac_v2_hip import ApproxContainer
    from plugin import create_evaluator, create_sampler

    kw = hip_kwargs(3, 1, (32, 32), 16, act_limit=2.0, env_id="synth_pendulum", sample_batch_size=20, reward_scale=1,
                    buffer_warm_size=100, max_iteration=12, log_save_interval=4, apprfunc_save_interval=4, eval_interval=6,
                    num_eval_episode=1, ini_network_dir=None, save_folder=str(tmp_path / name), seed=3, buffer_max_size=150)
    kw.update(over)
    torch.manual_seed(0)
    np.random.seed(0)
    nets = ApproxContainer(**kw)
    sampler = create_sampler(env=env if env is not None else _pendulum(), **kw)
    buf = HipReplayBuffer(hip_engine=StandInEngine(3, 1, 16), **kw)
    return kw, StubAlg(nets), sampler, buf, create_evaluator(**kw)


def test_an_environment_without_the_two_methods_is_named():
    from training.hip_sampler import HipOffSampler
    from training.hip_tensor_sampler import HipTensorEnvSampler

    smp = HipOffSampler(env=_pendulum(with_state=False), sample_batch_size=4)
    with pytest.raises(NotImplementedError, match=r"state_dict\(\).*load_state_dict\(sd\)"):
        smp.run_state()
    with pytest.raises(NotImplementedError, match=r"state_dict\(\).*load_state_dict\(sd\)"):
        smp.load_run_state({})

    class TensorEnv:
        num_envs = 4

    with pytest.raises(NotImplementedError, match=r"state_dict\(\).*load_state_dict\(sd\)"):
        HipTensorEnvSampler(env=TensorEnv(), sample_batch_size=8).run_state()
    sd = HipOffSampler(env=_pendulum(), sample_batch_size=4).run_state()
    assert set(sd) == {"format", "total_sample_number", "obs", "info", "env"} and pickle.loads(pickle.dumps(sd))["env"]["t"] == 0


def test_run_state_directories(tmp_path, monkeypatch):
    from training.hip_trainer import HipOffSerialTrainer

    kw, alg, smp, buf, ev = _parts(tmp_path, "a", hip_save_run_state=True)
    tr = HipOffSerialTrainer(alg, smp, buf, ev, **kw)
    order = []
    real_rename = os.rename
    # every rename into place: the ring directory first, run.pkl last -- with everything else already there
    monkeypatch.setattr(os, "rename", lambda a, b: (order.append((os.path.basename(b), sorted(os.listdir(os.path.dirname(b))))),
                                                   real_rename(a, b))[1])
    seen = []
    for it in range(12):
        tr.iteration = it
        tr.step()
        d = tmp_path / "a" / "apprfunc"
        seen.append(sorted(fn for fn in os.listdir(d) if fn.startswith("run_state_")))
    # a directory at the save iterations only; hip_run_state_keep = 1: the older one goes once the newer is complete
    assert seen == [["run_state_0"]] * 4 + [["run_state_4"]] * 4 + [["run_state_8"]] * 4
    d8 = tmp_path / "a" / "apprfunc" / "run_state_8"
    assert sorted(os.listdir(d8)) == ["networks.pkl", "optstate.pkl", "ring", "run.pkl"]
    # run.pkl was written last: everything else was there when it was opened
    assert [o[0] for o in order[-2:]] == ["ring", "run.pkl"] and order[-1][1] == ["networks.pkl", "optstate.pkl", "ring", "run.pkl.tmp"]
    run = pickle.load(open(d8 / "run.pkl", "rb"))
    assert run["format"] == "dsact-run-state/1" and run["next_iteration"] == 9
    assert run["fingerprint"] == {"algorithm": "StubAlg", "replay_batch_size": 16, "sample_interval": 1, "seed": 3, "strict_rng": False,
                                  "hip_device_indices": False}
    assert run["sampler"]["total_sample_number"] == 100 + 9 * 20 and run["numpy_rng"][0] == "MT19937"   # warm-up + iterations 0 .. 8
    assert json.load(open(d8 / "ring" / "meta.json"))["size"] == buf.size == 150

    # keep = 2
    kw2, alg2, smp2, buf2, ev2 = _parts(tmp_path, "b", hip_save_run_state=True, hip_run_state_keep=2)
    HipOffSerialTrainer(alg2, smp2, buf2, ev2, **kw2).train()
    assert sorted(fn for fn in os.listdir(tmp_path / "b" / "apprfunc") if fn.startswith("run_state_")) == ["run_state_12", "run_state_8"]
    assert pickle.load(open(tmp_path / "b" / "apprfunc" / "run_state_12" / "run.pkl", "rb"))["next_iteration"] == 12   # after the last iteration

    # without the kwarg nothing of this is written
    kw3, alg3, smp3, buf3, ev3 = _parts(tmp_path, "c")
    HipOffSerialTrainer(alg3, smp3, buf3, ev3, **kw3).train()
    assert not [fn for fn in os.listdir(tmp_path / "c" / "apprfunc") if fn.startswith("run_state_")]


def test_a_resumed_trainer_continues_and_refuses_another_run(tmp_path):
    from training.hip_trainer import HipOffSerialTrainer

    kw, alg, smp, buf, ev = _parts(tmp_path, "a", hip_save_run_state=True, hip_run_state_keep=8)
    tr = HipOffSerialTrainer(alg, smp, buf, ev, **kw)
    tr.train()
    d = str(tmp_path / "a" / "apprfunc" / "run_state_4")
    saved = pickle.load(open(os.path.join(d, "run.pkl"), "rb"))
    kw2, alg2, smp2, buf2, ev2 = _parts(tmp_path, "b", ini_run_state_dir=d)
    torch.manual_seed(77)                                            # whatever was drawn before: the saved states come last
    tr2 = HipOffSerialTrainer(alg2, smp2, buf2, ev2, **kw2)
    assert tr2.iteration == 5 and alg2.loaded["calls"] == 5
    assert smp2.get_total_sample_number() == saved["sampler"]["total_sample_number"]      # the warm-up loop sampled nothing
    assert np.array_equal(smp2.obs, saved["sampler"]["obs"]) and smp2.env.state_dict() == saved["sampler"]["env"]
    assert torch.equal(torch.get_rng_state(), saved["torch_rng"])
    got = np.random.get_state()
    assert got[0] == saved["numpy_rng"][0] and np.array_equal(got[1], saved["numpy_rng"][1]) and got[2:] == saved["numpy_rng"][2:]
    assert buf2.engine.buffer_digest(0, buf2.size) == ring_digest_reference(
        {k: np.fromfile(os.path.join(d, "ring", k + ".bin"), np.float32).reshape(buf2.size, -1 if k in ("obs", "obs2", "act") else 1)
         for k in RING_COLUMNS}, 0)
    # a run that starts at iteration 0 opens the log with two lines at step 0; this one does not
    assert not os.path.exists(tmp_path / "b" / "scalars.jsonl") or not open(tmp_path / "b" / "scalars.jsonl").read()
    tr2.train()
    assert alg2.calls == list(range(5, 12))
    for key, val in (("replay_batch_size", 32), ("sample_interval", 2), ("seed", 4), ("strict_rng", True)):
        kw3, alg3, smp3, buf3, ev3 = _parts(tmp_path, "c_" + key, ini_run_state_dir=d)
        kw3[key] = val
        with pytest.raises(ValueError, match=key):
            HipOffSerialTrainer(alg3, smp3, buf3, ev3, **kw3)
    with pytest.raises(ValueError, match="run.pkl"):
        kw4, alg4, smp4, buf4, ev4 = _parts(tmp_path, "d", ini_run_state_dir=str(tmp_path))
        HipOffSerialTrainer(alg4, smp4, buf4, ev4, **kw4)


def test_setups_that_cannot_be_carried_are_refused(tmp_path):
    from training.hip_async_trainer import HipOffAsyncTrainer
    from training.hip_trainer import HipOffSerialTrainer
    from training.hip_vec_sampler import HipVecOffSampler

    for k, v in (("hip_save_run_state", True), ("ini_run_state_dir", str(tmp_path))):
        kw, alg, smp, buf, ev = _parts(tmp_path, "a", **{k: v})
        with pytest.raises(NotImplementedError, match=k):
            HipOffAsyncTrainer(alg, smp, buf, ev, **kw)

        class NoRunState:
            networks = None

            def sample(self):
                raise AssertionError("refused before anything is sampled")

        with pytest.raises(NotImplementedError, match="run_state"):
            HipOffSerialTrainer(alg, NoRunState(), buf, ev, **kw)

        class NoSidecar:
            networks = alg.networks

        with pytest.raises(NotImplementedError, match="optimizer_state_dict"):
            HipOffSerialTrainer(NoSidecar(), smp, buf, ev, **kw)

        class NoSave:
            size = 1000

        with pytest.raises(NotImplementedError, match="save"):
            HipOffSerialTrainer(alg, smp, NoSave(), ev, **kw)
    assert not hasattr(HipVecOffSampler, "run_state")
