"""Episode statistics of the device-resident sampler's training environments (dsact_track_begin / dsact_track_commit /
dsact_track_read, training/hip_tensor_sampler.py with hip_episode_stats) -- the host side, without a GPU.

  1. the three entry points are declared, exported and bound; NULL-handle calls refuse;
  2. two statements of the bookkeeping, used here and by tests/test_episode_stats_gpu.py:
       TrackBook        the kernel's rule over whole NumPy columns (the state machine, step by step);
       reference_state  the yardstick: per environment, one episode at a time, the rewards added one by one in float64
                        (training/evaluator.py's sum(reward_list), written as a loop: Python's `sum` compensates float sums
                        from 3.12 on);
     they agree bit for bit on scripted data;
  3. the sampler on a recording fake engine: no track_* call without the kwarg, one track_begin and one track_commit per
     sample() with it, refusals before any environment or engine call;
  4. the sampler's loop over tests/envs/synth_tensor_episodes.py on a fake engine whose track_commit is TrackBook, against
     reference_state and the fixture's episode_plan;
  5. the aggregation (zero episodes: nan; exactly rounded means) and the K-th-call keys.
  6. HipOffSerialTrainer.step() with K > 1: which reads reach the writer, with and without `sample_calls` set.
"""
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "dsac-v2_amd")
for _p in (ROOT, PKG, HERE, os.path.join(HERE, "envs")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_tensor_sampler_host import FakeEngine as _ActingFake   # noqa: E402

COLUMNS = (("episodes", np.int64), ("terminated", np.int64), ("ret_sum", np.float64), ("ret_min", np.float64),
           ("ret_max", np.float64), ("len_sum", np.int64), ("last_ret", np.float64), ("last_len", np.int32),
           ("cur_ret", np.float64), ("cur_len", np.int32))
TB_KEYS = ["Sampler/episodes", "Sampler/episode return mean", "Sampler/episode return min", "Sampler/episode return max",
           "Sampler/episode length mean", "Sampler/terminated share"]
TIME_KEY = "Time/Sampler time [ms]-RL iter"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same_state(got, want, where=None):
    """every column: the same dtype, fp64 as bit patterns, the integers exactly"""
    assert list(got) == [k for k, _ in COLUMNS] == list(want), where
    for k, dt in COLUMNS:
        assert got[k].dtype == dt and want[k].dtype == dt, (k, where)
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, where, got[k], want[k])


# ---- 1. the C-ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    import ctypes as C

    from dsact import _ffi
    from dsact.engine import DsactEngine

    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    P, I = C.c_void_p, C.c_int32
    want = {
        "dsact_track_begin": (r"int dsact_track_begin\(dsact_handle\* h, int32_t n_envs\);", [P, I]),
        "dsact_track_commit": (r"int dsact_track_commit\(dsact_handle\* h, const float\* reward_dev, const uint8_t\* terminated_dev, "
                               r"const uint8_t\* truncated_dev,\s+int32_t n_steps\);", [P, P, P, P, I]),
        "dsact_track_read": (r"int dsact_track_read\(dsact_handle\* h, int32_t n_envs, int64_t\* episodes, int64_t\* terminated, "
                             r"double\* ret_sum, double\* ret_min,\s+double\* ret_max, int64_t\* len_sum, double\* last_ret, "
                             r"int32_t\* last_len, double\* cur_ret, int32_t\* cur_len,\s+int32_t clear\);",
                             [P, I] + [P] * 10 + [I]),
    }
    bound = {n: (res, args) for n, res, args in _ffi.SYMBOLS}
    for name, (decl, args) in want.items():
        assert re.search(decl, hdr), name
        assert bound[name] == (C.c_int, args), name
    # the wrapper hands dsact_track_read its arrays in the prototype's order
    order = re.search(r"int dsact_track_read\(([^;]*)\);", hdr).group(1)
    assert re.findall(r"\*\s*(\w+)", order)[1:] == [k for k, _ in DsactEngine.TRACK_COLUMNS] == [k for k, _ in COLUMNS]
    assert [np.dtype(d) for _, d in DsactEngine.TRACK_COLUMNS] == [np.dtype(d) for _, d in COLUMNS]
    lib = _ffi.load()
    for name in want:
        assert hasattr(lib, name), name
    # without a handle the entry points refuse like every other one
    assert lib.dsact_track_begin(None, 4) == -1
    assert lib.dsact_track_commit(None, None, None, None, 1) == -1
    assert lib.dsact_track_read(None, 4, *([None] * 10), 1) == -1


# ---- 2. the two statements ---------------------------------------------------------------------------------------------------------
class TrackBook:
    """k_track_commit / k_track_init over whole columns: the state machine, one lockstep step at a time"""

    def __init__(self, n):
        self.n = n
        self.s = {k: np.zeros(n, dt) for k, dt in COLUMNS}
        self.clear()

    def clear(self):
        s = self.s
        for k in ("episodes", "terminated", "len_sum", "last_len"):
            s[k][:] = 0
        s["ret_sum"][:] = 0.0
        s["last_ret"][:] = 0.0
        s["ret_min"][:] = np.inf
        s["ret_max"][:] = -np.inf

    def commit(self, rew, term, trunc, n_steps):
        s, n = self.s, self.n
        rew = np.asarray(rew, np.float32).reshape(n_steps, n)
        term, trunc = np.asarray(term).reshape(n_steps, n) != 0, np.asarray(trunc).reshape(n_steps, n) != 0
        for t in range(n_steps):
            s["cur_ret"] += rew[t].astype(np.float64)
            s["cur_len"] += 1
            end = term[t] | trunc[t]
            ret, ln = s["cur_ret"], s["cur_len"]
            s["episodes"] += end
            s["terminated"] += term[t]
            s["ret_sum"] = np.where(end, s["ret_sum"] + ret, s["ret_sum"])
            s["ret_min"] = np.where(end & (ret < s["ret_min"]), ret, s["ret_min"])
            s["ret_max"] = np.where(end & (ret > s["ret_max"]), ret, s["ret_max"])
            s["len_sum"] += np.where(end, ln, 0)
            s["last_ret"] = np.where(end, ret, s["last_ret"])
            s["last_len"] = np.where(end, ln, s["last_len"]).astype(np.int32)
            s["cur_ret"] = np.where(end, 0.0, ret)
            s["cur_len"] = np.where(end, 0, ln).astype(np.int32)

    def read(self, clear):
        out = {k: self.s[k].copy() for k, _ in COLUMNS}
        if clear:
            self.clear()
        return out


def reference_state(rew, term, trunc, clear_step=0):
    """the yardstick. rew / term / trunc [T, N]: every lockstep step so far. Per environment its episodes are cut out one at a
    time and each episode's rewards added one by one in float64; the totals hold the episodes that ENDED at a step >= clear_step
    (the steps before it were behind a clearing read), the episode in progress is whole whatever was cleared."""
    rew = np.asarray(rew, np.float32)
    T, N = rew.shape
    out = {k: np.zeros(N, dt) for k, dt in COLUMNS}
    out["ret_min"][:], out["ret_max"][:] = np.inf, -np.inf
    for i in range(N):
        start = 0
        for t in range(T):
            if term[t, i] or trunc[t, i]:
                ret = 0.0
                for s in range(start, t + 1):
                    ret += float(rew[s, i])
                length, start = t + 1 - start, t + 1
                if t < clear_step:
                    continue
                out["episodes"][i] += 1
                out["terminated"][i] += 1 if term[t, i] else 0
                out["ret_sum"][i] += ret
                if ret < out["ret_min"][i]:
                    out["ret_min"][i] = ret
                if ret > out["ret_max"][i]:
                    out["ret_max"][i] = ret
                out["len_sum"][i] += length
                out["last_ret"][i], out["last_len"][i] = ret, length
        ret = 0.0
        for s in range(start, T):
            ret += float(rew[s, i])
        out["cur_ret"][i], out["cur_len"][i] = ret, T - start
    return out


def scripted(T, N, seed):
    """rewards of magnitudes 1e-3 .. 1e3 (an fp32 running sum would round differently), flags with both kinds of end. Where N
    allows: row 1 ends at every step, row 2 never ends, row 0 ends with BOTH flags set at step 1."""
    g = torch.Generator().manual_seed(seed)
    rew = (torch.randn(T, N, generator=g) * torch.tensor(10.0) ** torch.randint(-3, 4, (T, N), generator=g).float()).contiguous()
    term, trunc = torch.rand(T, N, generator=g) < 0.15, torch.rand(T, N, generator=g) < 0.15
    if N > 1:
        term[::2, 1], trunc[1::2, 1] = True, True
    if N > 2:
        term[:, 2] = trunc[:, 2] = False
    if T > 1:
        term[1, 0] = trunc[1, 0] = True
    return rew, term, trunc


@pytest.mark.parametrize("N,T,chunk", [(1, 9, 1), (5, 24, 3), (33, 24, 8), (300, 16, 16)])
def test_state_machine_equals_the_per_environment_computation(N, T, chunk):
    rew, term, trunc = (x.numpy() for x in scripted(T, N, 10 * N + T))
    book = TrackBook(N)
    assert_same_state(book.read(False), reference_state(rew[:0], term[:0], trunc[:0]))
    clear_step = 0
    for c in range(T // chunk):
        r0, r1 = c * chunk, (c + 1) * chunk
        book.commit(rew[r0:r1].reshape(-1), term[r0:r1].reshape(-1), trunc[r0:r1].reshape(-1), chunk)
        want = reference_state(rew[:r1], term[:r1], trunc[:r1], clear_step)
        clear = c == T // chunk // 2
        assert_same_state(book.read(clear), want, (c, clear))
        if clear:
            clear_step = r1
            after = book.read(False)
            assert not after["episodes"].any() and np.isposinf(after["ret_min"]).all() and np.isneginf(after["ret_max"]).all()
            assert np.array_equal(bits(after["cur_ret"]), bits(want["cur_ret"])) and np.array_equal(after["cur_len"], want["cur_len"])
    final = book.read(False)
    if N >= 5:
        assert final["cur_len"][2] == T and final["episodes"][2] == 0                # the row that never ends
        assert final["cur_len"][1] == 0 and final["episodes"][1] == T - clear_step   # the row of length-1 episodes
    # the fp64 sum is what is held: an fp32 running sum of the same rewards differs somewhere
    acc = np.zeros(N, np.float32)
    for t in range(T):
        acc = np.where(term[t] | trunc[t], np.float32(0), acc + rew[t])
    if N >= 5:
        assert (acc.astype(np.float64) != final["cur_ret"]).any()


# ---- 3. the sampler's calls ----------------------------------------------------------------------------------------------------------
class RecordingEngine(_ActingFake):
    """the sampler host test's fake (a fixed 'policy', every call recorded) plus the three statistics calls, served by TrackBook"""

    def __init__(self, obs_dim, act_dim):
        super().__init__(obs_dim=obs_dim, act_dim=act_dim)
        self.book = None

    def track_begin(self, n_envs):
        self.calls.append(("track_begin", int(n_envs)))
        self.book = TrackBook(int(n_envs))

    def track_commit(self, reward, terminated, truncated, n_steps):
        assert reward.dtype == torch.float32 and terminated.dtype == truncated.dtype == torch.bool
        assert reward.shape == terminated.shape == truncated.shape == (n_steps * self.book.n,)
        self.calls.append(("track_commit", int(n_steps)))
        self.book.commit(reward.numpy(), terminated.numpy(), truncated.numpy(), n_steps)

    def track_read(self, clear=True):
        self.calls.append(("track_read", bool(clear)))
        return self.book.read(clear)


def _sampler(N, S, **over):
    from plugin import create_sampler
    from synth_tensor_episodes import A, O, SynthTensorEpisodes

    eng = RecordingEngine(O, A)
    smp = create_sampler(sampler_name="hip_tensor_env_sampler", env=SynthTensorEpisodes(N), sample_batch_size=S,
                         networks=types.SimpleNamespace(policy=types.SimpleNamespace(_engine=eng)), seed=3, **over)
    return smp, eng


def _track_calls(eng):
    return [c for c in eng.calls if c[0].startswith("track_")]


def test_without_the_kwarg_nothing_changes():
    smp, eng = _sampler(5, 15)
    for _ in range(3):
        _, tb = smp.sample()
        assert list(tb) == [TIME_KEY]
    assert _track_calls(eng) == [] and [c[0] for c in eng.calls] == ["set_act_rng"] + ["act_sample_device"] * 9
    with pytest.raises(RuntimeError, match="hip_episode_stats"):
        smp.episode_statistics()
    assert _track_calls(eng) == []
    smp, eng = _sampler(5, 15, hip_episode_stats=False, hip_episode_stats_every=0)
    smp.sample()
    assert _track_calls(eng) == []


@pytest.mark.parametrize("N,S", [(5, 5), (5, 15), (33, 66)])
def test_one_begin_and_one_commit_per_sample(N, S):
    smp, eng = _sampler(N, S, hip_episode_stats=True)
    assert _track_calls(eng) == []                                  # nothing before the first sample()
    for _ in range(4):
        _, tb = smp.sample()
        assert list(tb) == [TIME_KEY]                               # K = 0: sample() never reads
    assert _track_calls(eng) == [("track_begin", N)] + [("track_commit", S // N)] * 4
    names = [c[0] for c in eng.calls]
    assert names.index("track_begin") < names.index("act_sample_device")
    per_call = 1 + S // N                                           # the commit comes after the loop of every sample()
    assert [n for n in names if n in ("act_sample_device", "track_commit")] == (["act_sample_device"] * (S // N) + ["track_commit"]) * 4
    assert len(names) == 2 + 4 * per_call
    stats = smp.episode_statistics(clear=False)
    assert _track_calls(eng)[-1] == ("track_read", False) and set(stats) == {
        "episodes", "terminated_share", "return_mean", "return_min", "return_max", "length_mean", "rows"}
    smp.episode_statistics()
    assert _track_calls(eng)[-1] == ("track_read", True)            # clearing is the default
    # a new engine starts new statistics
    eng2 = RecordingEngine(eng.obs_dim, eng.act_dim)
    smp.networks = types.SimpleNamespace(policy=types.SimpleNamespace(_engine=eng2))
    smp.sample()
    assert _track_calls(eng2) == [("track_begin", N), ("track_commit", S // N)]


def test_constructor_refusals_come_before_anything_runs():
    from plugin import create_sampler
    from synth_tensor_episodes import A, O

    class NoCalls(RecordingEngine):
        def act_sample_device(self, *a, **k):
            raise AssertionError("an engine call before the refusal")

        set_act_rng = track_begin = track_commit = track_read = act_sample_device

    class NoEnv:
        def __getattr__(self, k):
            raise AssertionError("environment call %s before the refusal" % k)

    base = dict(sampler_name="hip_tensor_env_sampler", env=NoEnv(), sample_batch_size=32,
                networks=types.SimpleNamespace(policy=types.SimpleNamespace(_engine=NoCalls(O, A))))
    with pytest.raises(ValueError, match="hip_episode_stats_every"):
        create_sampler(**dict(base, hip_episode_stats=True, hip_episode_stats_every=-1))
    with pytest.raises(ValueError, match="hip_episode_stats_every"):
        create_sampler(**dict(base, hip_episode_stats=True, hip_episode_stats_every=2.5))
    with pytest.raises(ValueError, match="needs hip_episode_stats=True"):
        create_sampler(**dict(base, hip_episode_stats_every=2))
    with pytest.raises(ValueError, match="needs hip_episode_stats=True"):
        create_sampler(**dict(base, hip_episode_stats=False, hip_episode_stats_every=1))


# ---- 4. the loop against the yardstick ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S", [(5, 5), (5, 15), (33, 66)])
def test_sampler_loop_equals_the_per_environment_computation(N, S):
    from synth_tensor_episodes import episode_plan

    steps = 30
    smp, eng = _sampler(N, S, hip_episode_stats=True, reward_scale=0.25)
    rew, term, trunc = [], [], []
    clear_step, calls = 0, steps // (S // N)
    for c in range(calls):
        batch, _ = smp.sample()
        rew.append(batch.rew.numpy().reshape(S // N, N).copy())
        term.append(batch.terminated.numpy().reshape(S // N, N).copy())
        trunc.append(batch.truncated.numpy().reshape(S // N, N).copy())
        R, TE, TR = np.concatenate(rew), np.concatenate(term), np.concatenate(trunc)
        clear = c == calls // 2
        got = smp.episode_statistics(clear=clear)
        assert_same_state(got["rows"], reference_state(R, TE, TR, clear_step), (c, clear))
        if clear:
            clear_step = len(R)
    assert len(R) == steps
    # what the fixture is here for: both kinds of end, both flags in one step, several rows ending together, length-1
    # episodes, a row with many episodes -- and rewards that are the environment's own (not scaled by reward_scale)
    end = TE | TR
    assert (TE & ~TR).any() and (TR & ~TE).any() and (TE & TR).any() and (end.sum(axis=1) > 1).any()
    whole = reference_state(R, TE, TR)
    assert whole["episodes"].max() >= 10 and whole["cur_len"].max() > 0 and (whole["episodes"] == 0).sum() == 0
    assert whole["terminated"].sum() == TE.sum()
    # ... and the plan the fixture publishes, in plain integers: episodes, lengths and kinds of end per row
    planned = []
    for r in range(N):
        k = t = n_term = 0
        while True:
            length, te, _ = episode_plan(r, k)
            if t + length > steps:
                break
            t, k, n_term = t + length, k + 1, n_term + int(te)
            planned.append(length)
        assert (whole["episodes"][r], whole["len_sum"][r], whole["terminated"][r], whole["cur_len"][r]) == (k, t, n_term, steps - t), r
    assert 1 in planned and max(planned) > 1
    # the reward table bounds the returns from above: the actions (|a|^2 >= 0) reached them
    assert np.isfinite(whole["ret_sum"]).all() and (whole["ret_max"] < 2.0 * 11).all()


# ---- 5. the aggregation and the K-th call ---------------------------------------------------------------------------------------------
def _rows(**cols):
    n = len(next(iter(cols.values())))
    rows = {k: np.zeros(n, dt) for k, dt in COLUMNS}
    rows["ret_min"][:], rows["ret_max"][:] = np.inf, -np.inf
    for k, v in cols.items():
        rows[k][:] = v
    return rows


def test_aggregation():
    from training.hip_tensor_sampler import aggregate_episode_rows

    none = aggregate_episode_rows(_rows(cur_ret=[1.5, 2.5], cur_len=[3, 4]))
    assert none["episodes"] == 0 and type(none["episodes"]) is int
    for k in ("terminated_share", "return_mean", "return_min", "return_max", "length_mean"):
        assert math.isnan(none[k]), k
    assert none["rows"]["cur_len"].tolist() == [3, 4]                # the episodes in progress are handed on
    # per-row sums whose left-to-right (and pairwise) float sum is not the rounded true sum; row 4 has no episode
    rows = _rows(episodes=[1, 2, 1, 3, 0], terminated=[1, 0, 0, 2, 0], ret_sum=[1e16, 1.0, -1e16, 1.0, 0.0],
                 ret_min=[1e16, -2.0, -1e16, 0.25, np.inf], ret_max=[1e16, 3.0, -1e16, 0.5, -np.inf], len_sum=[4, 9, 1, 7, 0])
    got = aggregate_episode_rows(rows)
    assert got["episodes"] == 7 and got["return_mean"] == 2.0 / 7 and got["return_mean"] == math.fsum(rows["ret_sum"].tolist()) / 7
    acc = 0.0
    for v in rows["ret_sum"]:
        acc += float(v)
    assert acc / 7 != got["return_mean"]                             # the one-by-one sum loses the two 1.0s
    assert got["return_min"] == -1e16 and got["return_max"] == 1e16
    assert got["length_mean"] == 21 / 7 and got["terminated_share"] == 3 / 7
    assert got["rows"] is rows
    # the order of the rows does not reach the result
    perm = [3, 0, 4, 2, 1]
    again = aggregate_episode_rows({k: v[perm] for k, v in rows.items()})
    assert all(again[k] == got[k] for k in got if k != "rows")


def test_kth_call_puts_the_keys_into_the_returned_dict():
    K, N, S = 3, 5, 15
    smp, eng = _sampler(N, S, hip_episode_stats=True, hip_episode_stats_every=K)
    seen = []
    for call in range(1, 8):
        reads = len([c for c in _track_calls(eng) if c[0] == "track_read"])
        _, tb = smp.sample()
        seen.append(sorted(tb))
        now = [c for c in _track_calls(eng) if c[0] == "track_read"]
        if call % K:
            assert list(tb) == [TIME_KEY] and len(now) == reads
            continue
        assert sorted(tb) == sorted(TB_KEYS + [TIME_KEY]) and now[reads:] == [("track_read", True)]       # ONE clearing read
        assert not eng.book.read(False)["episodes"].any()
        assert type(tb["Sampler/episodes"]) is int and tb["Sampler/episodes"] > 0
        assert tb["Sampler/episode return min"] <= tb["Sampler/episode return mean"] <= tb["Sampler/episode return max"]
        assert 1.0 <= tb["Sampler/episode length mean"] <= 11.0 and 0.0 <= tb["Sampler/terminated share"] <= 1.0
    assert [len(s) for s in seen] == [1, 1, 7, 1, 1, 7, 1]
    # K = 1: every call; the window of one call is what the call itself ended
    smp, eng = _sampler(N, S, hip_episode_stats=True, hip_episode_stats_every=1)
    for _ in range(3):
        batch, tb = smp.sample()
        assert tb["Sampler/episodes"] == int((batch.terminated | batch.truncated).sum())


# ---- 6. the K-th call under HipOffSerialTrainer ----------------------------------------------------------------------------------------
class _Writer:
    def __init__(self):
        self.rows = []

    def add_dict(self, d, step):
        self.rows.extend((k, v, step) for k, v in d.items())

    def add(self, tag, value, step):
        self.rows.append((tag, value, step))

    def flush(self):
        pass


class _Ring:
    """a buffer that counts: its size, and the episodes that ended in every batch it was handed"""

    def __init__(self):
        self.size, self.ended = 0, []

    def add_batch(self, batch):
        self.size += len(batch)
        self.ended.append(int((batch.terminated | batch.truncated).sum()))

    def sample_batch(self, n):
        return None


def _trainer(K, warm_calls, si, L, preset):
    """HipOffSerialTrainer over the fake engine, a counting buffer and a recording writer; `preset`: sample_calls = K - 1 after
    the constructor (INTEGRATION.md's advice). Returns (trainer, sampler, engine, buffer, writer)."""
    from training.hip_trainer import HipOffSerialTrainer

    N, S = 5, 15
    smp, eng = _sampler(N, S, hip_episode_stats=True, hip_episode_stats_every=K)
    alg = types.SimpleNamespace(networks=smp.networks, local_update=lambda batch, it: {"Loss/x": 0.0})
    ring = _Ring()
    tr = HipOffSerialTrainer(alg, smp, ring, None, replay_batch_size=4, max_iteration=10 ** 6, sample_interval=si, log_save_interval=L,
                             apprfunc_save_interval=10 ** 6, eval_interval=10 ** 6, buffer_warm_size=warm_calls * S)
    assert smp.sample_calls == warm_calls == len(ring.ended)           # the constructor's warm-up calls are counted
    tr.writer = _Writer()
    if preset:
        smp.sample_calls = K - 1
    return tr, smp, eng, ring, tr.writer


def _drive(tr, iters):
    for _ in range(iters):
        tr.step()
        tr.iteration += 1


def test_trainer_with_k_above_one_writes_every_read_when_the_count_is_set():
    K, W, si, L, iters = 4, 2, 2, 8, 25                                 # K = L / si
    tr, smp, eng, ring, wr = _trainer(K, W, si, L, preset=True)
    _drive(tr, iters)
    episodes = [(v, step) for k, v, step in wr.rows if k == "Sampler/episodes"]
    assert [step for _, step in episodes] == [0, 8, 16, 24]             # every log iteration
    reads = [c for c in _track_calls(eng) if c[0] == "track_read"]
    assert reads == [("track_read", True)] * 4                          # ... and no read besides them: nothing is dropped
    for key in TB_KEYS:
        assert [step for k, _, step in wr.rows if k == key] == [0, 8, 16, 24], key
    # each read covers the sample() calls since the one before; the first one the warm-up's too
    assert len(ring.ended) == W + 13
    want = [sum(ring.ended[:W + 1])] + [sum(ring.ended[W + 1 + 4 * j:W + 5 + 4 * j]) for j in range(3)]
    assert [v for v, _ in episodes] == want and sum(want) == sum(ring.ended) > 0


def test_trainer_without_setting_the_count_follows_the_stated_arithmetic():
    K, W, si, L, iters = 3, 2, 2, 8, 25
    tr, smp, eng, ring, wr = _trainer(K, W, si, L, preset=False)
    _drive(tr, iters)
    # the call of iteration `it` is call W + it / si + 1: a read where K divides it, written down at log iterations only
    read_its = [it for it in range(0, iters, si) if (W + it // si + 1) % K == 0]
    assert read_its == [0, 6, 12, 18, 24]
    assert [c for c in _track_calls(eng) if c[0] == "track_read"] == [("track_read", True)] * len(read_its)
    assert [step for k, _, step in wr.rows if k == "Sampler/episodes"] == [it for it in read_its if it % L == 0] == [0, 24]
