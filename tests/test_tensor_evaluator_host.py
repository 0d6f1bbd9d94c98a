"""Device-resident evaluator for batched tensor environments (training/hip_tensor_evaluator.py, dsact_act_mode_device /
dsact_eval_begin / dsact_eval_commit / dsact_eval_poll / dsact_eval_read) -- the host side, without a GPU.

  1. the five entry points are declared, exported and bound; without a handle they refuse;
  2. plugin.create_evaluator routes by evaluator_name and leaves every other name where it was;
  3. every refusal comes before any environment or engine call;
  4. the fixture tests/envs/synth_tensor_episodes.py: its ends are what `episode_plan` says, and the plans hold every case the GPU
     tests rely on;
  5. the evaluator's loop on a fake engine whose eval_commit is the NumPy restatement of k_eval_commit: returns and lengths
     against an independent computation (one environment object per row, one episode at a time), poll periods, the clip, the
     step cap.
"""
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
for _p in (ROOT, PKG, os.path.join(HERE, "envs")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

O, A = 17, 6
CASES = [(5, 3), (5, 7), (5, 70), (33, 40)]


# ---- 1. the C-ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    import ctypes as C

    from dsact import _ffi

    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    P = C.c_void_p
    want = {
        "dsact_act_mode_device": (r"int dsact_act_mode_device\(dsact_handle\* h, const float\* obs_dev, int32_t n, float\* action_dev\);",
                                  [P, P, C.c_int32, P]),
        "dsact_eval_begin": (r"int dsact_eval_begin\(dsact_handle\* h, int32_t n_envs, int32_t n_episodes\);", [P, C.c_int32, C.c_int32]),
        "dsact_eval_commit": (r"int dsact_eval_commit\(dsact_handle\* h, const float\* reward_dev, const uint8_t\* terminated_dev, "
                              r"const uint8_t\* truncated_dev,\s+uint8_t\* ended_dev\);", [P, P, P, P, P]),
        "dsact_eval_poll": (r"int dsact_eval_poll\(dsact_handle\* h, int32_t\* remaining\);", [P, P]),
        "dsact_eval_read": (r"int dsact_eval_read\(dsact_handle\* h, double\* returns, int32_t\* lengths, int32_t n_episodes\);",
                            [P, P, P, C.c_int32]),
    }
    bound = {n: (res, args) for n, res, args in _ffi.SYMBOLS}
    for name, (decl, args) in want.items():
        assert re.search(decl, hdr), name
        assert bound[name] == (C.c_int, args), name
    doc = hdr[hdr.index("Device-resident evaluation"):hdr.index("int dsact_act_mode_device")]
    for name in want:      # each entry says which reference lines it replaces
        entry = doc[doc.index("*   " + name):]
        assert "training/evaluator.py:34-84" in entry[:700], name
    lib = _ffi.load()
    for name in want:
        assert hasattr(lib, name), name
    # without a handle the entry points refuse like every other one
    assert lib.dsact_act_mode_device(None, None, 1, None) == -1
    assert lib.dsact_eval_begin(None, 1, 1) == -1
    assert lib.dsact_eval_commit(None, None, None, None, None) == -1
    assert lib.dsact_eval_poll(None, None) == -1
    assert lib.dsact_eval_read(None, None, None, 1) == -1


# ---- the fake engine ----------------------------------------------------------------------------------------------------------------
class FakeEngine:
    """records the calls the evaluator makes. Its 'policy' is a fixed, exactly representable function of the observation; its
    eval_* are the NumPy restatement of include/dsact.h's description of k_eval_commit. No GPU."""
    conv_type = None

    def __init__(self, obs_dim=O, act_dim=A, limit=0.4):
        self.obs_dim, self.act_dim = obs_dim, act_dim
        self.device = torch.device("cpu")
        self.act_low, self.act_high = np.full(act_dim, -limit, np.float32), np.full(act_dim, limit, np.float32)
        self.calls = []
        self.ep = None

    def note_torch_writes(self, params):
        self.calls.append(("note_torch_writes",))

    def act_mode_device(self, obs, action):
        n = obs.shape[0]
        assert obs.shape == (n, self.obs_dim) and action.shape == (n, self.act_dim) and obs.dtype == action.dtype == torch.float32
        action.copy_(obs[:, :self.act_dim] * 0.375)          # |.| <= 0.375: inside the +-0.4 limits, exact in fp32
        self.calls.append(("act_mode_device", n))

    def eval_begin(self, n, e):
        self.N, self.E = n, e
        self.ep = np.where(np.arange(n) < e, np.arange(n), -1).astype(np.int32)
        self.acc, self.len = np.zeros(n, np.float64), np.zeros(n, np.int32)
        self.returns, self.lengths = np.zeros(e, np.float64), np.zeros(e, np.int32)
        self.remaining = e
        self.calls.append(("eval_begin", n, e))

    def eval_commit(self, reward, terminated, truncated, ended):
        assert reward.dtype == torch.float32 and terminated.dtype == truncated.dtype == ended.dtype == torch.bool
        assert reward.shape == terminated.shape == truncated.shape == ended.shape == (self.N,)
        rew, te, tr = reward.numpy(), terminated.numpy(), truncated.numpy()
        for i in range(self.N):
            end = bool(te[i]) | bool(tr[i])
            ended[i] = end
            if self.ep[i] >= 0:
                self.acc[i] += np.float64(rew[i])
                self.len[i] += 1
                if end:
                    e = self.ep[i]
                    self.returns[e], self.lengths[e] = self.acc[i], self.len[i]
                    self.acc[i], self.len[i] = 0.0, 0
                    self.ep[i] = e + self.N if e + self.N < self.E else -1
                    self.remaining -= 1
        self.calls.append(("eval_commit",))

    def eval_poll(self):
        self.calls.append(("eval_poll",))
        return self.remaining

    def eval_read(self, e):
        assert e == self.E and self.remaining == 0
        self.calls.append(("eval_read", e))
        return self.returns.copy(), self.lengths.copy()


def _networks(eng):
    return types.SimpleNamespace(policy=types.SimpleNamespace(_engine=eng, parameters=lambda: []))


def _evaluator(N, E, eng=None, env=None, **over):
    from plugin import create_evaluator
    from synth_tensor_episodes import SynthTensorEpisodes

    eng = eng or FakeEngine()
    env = env or SynthTensorEpisodes(N)
    ev = create_evaluator(evaluator_name="hip_tensor_env_evaluator", eval_env=env, num_eval_episode=E, networks=_networks(eng), **over)
    return ev, eng, env


def _independent(N, E, lo=-0.4, hi=0.4):
    """the same evaluation with ONE environment object per row, one episode after the other: (returns, lengths, lockstep steps
    the slowest row needs)"""
    from synth_tensor_episodes import SynthTensorEpisodes

    eng = FakeEngine()
    returns, lengths, busiest = np.zeros(E, np.float64), np.zeros(E, np.int32), 0
    for r in range(min(N, E)):
        env = SynthTensorEpisodes(1, env_offset=r)
        obs = env.reset()
        total = 0
        for e in range(r, E, N):
            acc, n = np.float64(0.0), 0
            while True:
                a = torch.empty(1, A)
                eng.act_mode_device(obs, a)
                obs2, rew, term, trunc = env.step(a.clamp(lo, hi))
                acc, n = acc + np.float64(rew.numpy()[0]), n + 1
                end = term | trunc
                obs = env.reset(end)
                if bool(end):
                    break
            returns[e], lengths[e], total = acc, n, total + n
        busiest = max(busiest, total)
    return returns, lengths, busiest


# ---- 2. routing --------------------------------------------------------------------------------------------------------------------
def test_create_evaluator_routes_by_name_and_leaves_the_others():
    from plugin import create_evaluator
    from training.hip_tensor_evaluator import HipTensorEnvEvaluator
    from training.hip_trainer import HipEvaluator
    from training.hip_vec_evaluator import HipVecEvaluator

    ev, _, env = _evaluator(5, 3)
    assert type(ev) is HipTensorEnvEvaluator and ev.env is env and ev.poll_steps == 16 and ev.max_steps == 100000
    gym = types.SimpleNamespace(reset=lambda: np.zeros(3, np.float32))
    for name in (None, "evaluator", "hip_evaluator", "anything"):
        kw = {} if name is None else {"evaluator_name": name}
        assert type(create_evaluator(eval_env=gym, **kw)) is HipEvaluator, name
        assert type(create_evaluator(eval_envs=[gym, gym], hip_eval_env_num=2, **kw)) is HipVecEvaluator, name
    # `env` when no eval_env is given (the reference's kwargs carry no eval_env)
    from synth_tensor_episodes import SynthTensorEpisodes
    env2 = SynthTensorEpisodes(4)
    assert create_evaluator(evaluator_name="hip_tensor_env_evaluator", env=env2, networks=_networks(FakeEngine())).env is env2


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_runs():
    from plugin import create_evaluator

    class NoCalls(FakeEngine):
        def act_mode_device(self, *a, **k):
            raise AssertionError("an engine call before the refusal")

        note_torch_writes = eval_begin = eval_commit = eval_poll = eval_read = act_mode_device

    class NoEnv:
        num_envs, action_low, action_high = 8, torch.full((A,), -0.4), torch.full((A,), 0.4)

        def __getattr__(self, k):
            raise AssertionError("environment call %s before the refusal" % k)

    base = dict(evaluator_name="hip_tensor_env_evaluator", eval_env=NoEnv(), num_eval_episode=4, networks=_networks(NoCalls()))
    with pytest.raises(ValueError, match="num_eval_episode"):
        create_evaluator(**dict(base, num_eval_episode=0))
    with pytest.raises(ValueError, match="hip_eval_poll_steps"):
        create_evaluator(**dict(base, hip_eval_poll_steps=0))
    with pytest.raises(NotImplementedError, match="attached"):
        create_evaluator(**dict(base, networks=types.SimpleNamespace(policy=torch.nn.Linear(2, 2))))
    cnn = NoCalls()
    cnn.conv_type = "type_2"
    with pytest.raises(NotImplementedError, match="CNN"):
        create_evaluator(**dict(base, networks=_networks(cnn)))
    with pytest.raises(NotImplementedError, match="continuous"):
        create_evaluator(**dict(base, action_type="discret"))
    other = NoCalls()
    other.device = torch.device("meta")
    with pytest.raises(ValueError, match="lives on"):
        create_evaluator(**dict(base, networks=_networks(other)))
    # networks assigned later (what the trainer does): the same refusals at run_evaluation, still before any step
    ev = create_evaluator(**dict(base, networks=None))
    with pytest.raises(NotImplementedError, match="attached"):
        ev.run_evaluation(0)
    ev.networks = _networks(cnn)
    with pytest.raises(NotImplementedError, match="CNN"):
        ev.run_evaluation(0)
    ev.networks = _networks(other)
    with pytest.raises(ValueError, match="lives on"):
        ev.run_evaluation(0)


# ---- 4. the fixture ----------------------------------------------------------------------------------------------------------------
def test_fixture_ends_are_the_arithmetic_plan_and_hold_every_case():
    from synth_tensor_episodes import SynthTensorEpisodes, episode_plan, limit_of

    assert {limit_of(r) for r in range(33)} == set(range(1, 12))
    # the plans of the evaluation cases: both kinds of end, both flags in one step, length 1, a row without an episode, a row
    # with more than 3 episodes
    plans = {(N, E): [episode_plan(e % N, e // N) for e in range(E)] for N, E in CASES}
    for N, E in CASES:
        kinds = {(te, tr) for _, te, tr in plans[(N, E)]}
        assert (True, False) in kinds and (False, True) in kinds, (N, E)
    for N, E in ((5, 70), (33, 40)):
        assert (True, True) in {(te, tr) for _, te, tr in plans[(N, E)]} and 1 in {n for n, _, _ in plans[(N, E)]}, (N, E)
    assert episode_plan(0, 3) == (4, True, True) and episode_plan(0, 4) == (1, True, False) and episode_plan(9, 0)[0] == 1
    assert CASES[0][1] < CASES[0][0] and 70 // 5 > 3
    # the environment does what the plan says, whatever the actions; rows do not depend on the batch around them
    big, small = SynthTensorEpisodes(33), SynthTensorEpisodes(3, env_offset=7)
    ob, os_ = big.reset(), small.reset()
    assert ob.shape == (33, O) and ob.dtype == torch.float32 and torch.equal(ob[7:10], os_)
    g = torch.Generator().manual_seed(1)
    k, t, same_step = [0] * 33, [0] * 33, 0
    for step in range(60):
        a = torch.rand(33, A, generator=g) * 0.8 - 0.4
        rb, rs = big.step(a), small.step(a[7:10])
        for x, y in zip(rb, rs):
            assert torch.equal(x[7:10], y), step
        obs2, rew, term, trunc = rb
        assert rew.dtype == torch.float32 and term.dtype == trunc.dtype == torch.bool
        for r in range(33):
            t[r] += 1
            n, te, tr = episode_plan(r, k[r])
            assert (bool(term[r]), bool(trunc[r])) == ((te, tr) if t[r] == n else (False, False)), (step, r)
        sq = (a.double() ** 2).sum(dim=1)
        table = torch.tensor([((37 * r + 101 * t[r] + 11) % 64) / 16 - 2 for r in range(33)], dtype=torch.float64)
        assert float((rew.double() - (table - sq)).abs().max()) < 1e-6          # the actions reach the reward
        end = term | trunc
        same_step = max(same_step, int(end.sum()))
        for r in range(33):
            if bool(end[r]):
                k[r], t[r] = k[r] + 1, 0
        ob, os_ = big.reset(end), small.reset(rs[2] | rs[3])
        assert torch.equal(ob[7:10], os_) and torch.equal(ob[~end], obs2[~end])
    assert same_step >= 3                                                          # several rows end in the same step


# ---- 5. the loop -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E", CASES)
def test_loop_equals_the_independent_computation(N, E):
    from synth_tensor_episodes import episode_plan

    want_ret, want_len, busiest = _independent(N, E)
    assert [int(n) for n in want_len] == [episode_plan(e % N, e // N)[0] for e in range(E)]
    results = {}
    for P in (1, 7):
        ev, eng, _ = _evaluator(N, E, hip_eval_poll_steps=P)
        tar = ev.run_evaluation(0)
        assert ev.returns.dtype == np.float64 and ev.lengths.dtype == np.int32
        assert np.array_equal(ev.returns.view(np.uint64), want_ret.view(np.uint64)), P
        assert np.array_equal(ev.lengths, want_len), P
        assert tar == np.mean(want_ret)
        assert ev.steps == -(-busiest // P) * P                                    # it stops at the first poll that reads 0
        names = [c[0] for c in eng.calls]
        assert names[:2] == ["note_torch_writes", "eval_begin"] and eng.calls[1] == ("eval_begin", N, E)
        assert names.count("act_mode_device") == names.count("eval_commit") == ev.steps
        assert names.count("eval_poll") == ev.steps // P and names[-1] == "eval_read"
        assert all(c[1] == N for c in eng.calls if c[0] == "act_mode_device")    # ONE acting call per lockstep step, all rows
        # a second evaluation starts over
        assert ev.run_evaluation(1) == tar and np.array_equal(ev.lengths, want_len)
        results[P] = ev.steps
    assert abs(results[1] - results[7]) < 7


def test_environment_limits_other_than_the_policys_are_clipped_on_the_device():
    from synth_tensor_episodes import SynthTensorEpisodes

    N, E = 5, 7
    env = SynthTensorEpisodes(N)
    env.action_low, env.action_high = torch.full((N, A), -0.1), torch.full((N, A), 0.2)
    seen = []
    step = env.step
    env.step = lambda a: (seen.append(a.clone()), step(a))[1]
    ev, _, _ = _evaluator(N, E, env=env, hip_eval_poll_steps=1)
    ev.run_evaluation(0)
    assert float(torch.stack(seen).max()) == np.float32(0.2) and float(torch.stack(seen).min()) == np.float32(-0.1)
    want_ret, want_len, _ = _independent(N, E, lo=-0.1, hi=0.2)
    assert np.array_equal(ev.returns.view(np.uint64), want_ret.view(np.uint64)) and np.array_equal(ev.lengths, want_len)
    assert not np.array_equal(want_ret, _independent(N, E)[0])


def test_step_cap_raises_and_the_next_run_works():
    ev, eng, _ = _evaluator(5, 70, hip_eval_poll_steps=7, hip_eval_max_steps=10)
    with pytest.raises(RuntimeError, match="hip_eval_max_steps = 10"):
        ev.run_evaluation(0)
    names = [c[0] for c in eng.calls]
    assert ev.steps == 10 and names.count("eval_commit") == 10 and names.count("eval_poll") == 2 and "eval_read" not in names
    ev.max_steps = 100000
    assert ev.run_evaluation(0) == np.mean(_independent(5, 70)[0])
