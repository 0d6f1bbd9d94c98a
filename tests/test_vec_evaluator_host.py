"""HipVecEvaluator (training/hip_vec_evaluator.py) on CPU: unattached containers act through the module forward, so the
episode-to-environment assignment, the lockstep loop with its live-row compaction and the TAR's reduction order are
checked here against HipEvaluator without a GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dsac-v2_amd"))


class _Box:
    def __init__(self, lim, n):
        self.low, self.high = np.full(n, -lim, np.float32), np.full(n, lim, np.float32)


class _EpEnv:
    """environment k: episode j (its j-th reset) is truncated after 2 + k + (j % 3) steps, and every other episode of
    environment 1 terminates after 2 steps. The observation carries k and the step. action_reward=False: rewards and
    dynamics ignore the action; True: the reward is -|a - s[:A]|^2 with the observation moved by the action."""
    O, A = 5, 2

    def __init__(self, k, action_reward=False):
        self.k, self.action_reward = k, action_reward
        self.t, self.ep = 0, -1
        self.action_space = _Box(0.4, self.A)
        self.s = np.zeros(self.O, np.float32)
        self.lengths = []   # steps of every finished episode, in order

    def reset(self):
        self.t, self.ep = 0, self.ep + 1
        self.s = (np.linspace(-1, 1, self.O) * (1 + 0.1 * self.k) + 0.01 * self.ep).astype(np.float32)
        self.s[0] = self.k
        return self.s.copy(), {}

    def step(self, a):
        a = np.asarray(a, np.float32)
        assert a.shape == (self.A,)
        self.t += 1
        if self.action_reward:
            r = -float(np.sum((a - self.s[:self.A]) ** 2))
            self.s = (0.9 * self.s + 0.2 * np.resize(a, self.O)).astype(np.float32)
        else:
            r = float(np.float32(0.1) * self.s.sum() + 0.37 * self.t)
            self.s = (0.9 * self.s + 0.05).astype(np.float32)
        self.s[0] = self.k
        term = self.k == 1 and self.ep % 2 == 1 and self.t == 2
        trunc = self.t >= 2 + self.k + self.ep % 3
        if term or trunc:
            self.lengths.append(self.t)
        return self.s.copy(), r, term, {"TimeLimit.truncated": trunc}


def _nets(seed=0):
    from dsac_v2_hip import ApproxContainer

    torch.manual_seed(seed)
    return ApproxContainer(**hip_kwargs(_EpEnv.O, _EpEnv.A, (32, 32), 16, act_limit=0.4))


def _vec(envs, nets, E, **kw):
    from plugin import create_evaluator

    ev = create_evaluator(hip_eval_env_num=len(envs), eval_envs=envs, networks=nets, num_eval_episode=E, **kw)
    assert type(ev).__name__ == "HipVecEvaluator" and ev.route() == "module"
    return ev


def _separate(envs, nets, E):
    """HipEvaluator on a copy of every environment, given that environment's episodes (e % N == i) in order"""
    from training.hip_trainer import HipEvaluator

    N = len(envs)
    rets = [None] * E
    for i, env in enumerate(envs):
        mine = list(range(i, E, N))
        ev = HipEvaluator(eval_env=env, networks=nets, num_eval_episode=len(mine))
        for e in mine:
            rets[e] = ev.run_an_episode()
    return rets


def test_n1_or_absent_returns_hip_evaluator():
    from plugin import create_evaluator
    from training.hip_trainer import HipEvaluator
    from training.hip_vec_evaluator import HipVecEvaluator

    nets = _nets()
    for kw in ({}, {"hip_eval_env_num": 1}):
        ev = create_evaluator(env=_EpEnv(0), networks=nets, num_eval_episode=2, **kw)
        assert type(ev) is HipEvaluator
    ev = create_evaluator(hip_eval_env_num=2, eval_envs=[_EpEnv(0), _EpEnv(1)], networks=nets, num_eval_episode=2)
    assert type(ev) is HipVecEvaluator and ev.n_envs == 2


def test_bad_eval_envs_length_is_rejected():
    from plugin import create_evaluator
    from training.hip_vec_evaluator import HipVecEvaluator

    nets = _nets()
    for n in (1, 3):
        with pytest.raises(ValueError):
            create_evaluator(hip_eval_env_num=n, eval_envs=[_EpEnv(0), _EpEnv(1)], networks=nets)
    with pytest.raises(ValueError):
        HipVecEvaluator(hip_eval_env_num=3, eval_envs=[_EpEnv(0)], networks=nets)
    with pytest.raises(ValueError):
        HipVecEvaluator(hip_eval_env_num=0, networks=nets)


def test_episodes_run_on_environment_e_mod_n_in_order():
    N, E = 3, 8
    envs = [_EpEnv(k) for k in range(N)]
    ev = _vec(envs, _nets(), E)
    ev.run_evaluation(0)
    # environment i played episodes i, i + N, ... : its j-th episode is episode i + j N
    for i, env in enumerate(envs):
        mine = list(range(i, E, N))
        assert env.ep == len(mine) - 1
        assert env.lengths == [(2 if (i == 1 and j % 2 == 1) else 2 + i + j % 3) for j in range(len(mine))]
    assert all(r is not None for r in ev.returns) and len(ev.returns) == E
    # the lockstep loop runs as long as the busiest environment
    assert ev.steps == max(sum(env.lengths) for env in envs)


@pytest.mark.parametrize("N,E", [(3, 7), (4, 10), (2, 1), (5, 3)])
def test_tar_equals_separate_runs_bitwise_when_actions_do_not_matter(N, E):
    nets = _nets(1)
    vec = _vec([_EpEnv(k) for k in range(N)], nets, E)
    tar = vec.run_evaluation(0)
    rets = _separate([_EpEnv(k) for k in range(N)], nets, E)
    assert vec.returns == rets
    assert np.float64(tar).tobytes() == np.float64(np.mean(rets)).tobytes()


@pytest.mark.parametrize("N,E", [(3, 7), (4, 10)])
def test_tar_equals_separate_runs_with_action_dependent_rewards(N, E):
    nets = _nets(2)
    vec = _vec([_EpEnv(k, action_reward=True) for k in range(N)], nets, E)
    tar = vec.run_evaluation(0)
    rets = _separate([_EpEnv(k, action_reward=True) for k in range(N)], nets, E)
    np.testing.assert_allclose(vec.returns, rets, rtol=1e-5, atol=1e-6)
    assert abs(tar - np.mean(rets)) <= 1e-5 * abs(np.mean(rets)) + 1e-6


def test_live_rows_are_compacted_in_environment_order():
    N, E = 3, 5
    envs = [_EpEnv(k) for k in range(N)]
    nets = _nets()
    vec = _vec(envs, nets, E)
    seen = []
    h = nets.policy.register_forward_pre_hook(lambda _m, args: seen.append(args[0][:, 0].numpy().astype(int).tolist()))
    vec.run_evaluation(0)
    h.remove()
    # replay the schedule: environment i's episode lengths, its episodes e = i, i + N, ...
    remaining = {i: list(envs[i].lengths) for i in range(N)}
    left = {i: remaining[i].pop(0) for i in range(N)}
    want = []
    while left:
        live = sorted(left)
        want.append(live)
        for i in live:
            left[i] -= 1
            if left[i] == 0:
                if remaining[i]:
                    left[i] = remaining[i].pop(0)
                else:
                    del left[i]
    assert seen == want
    assert len(seen[0]) == N and min(len(r) for r in seen) < N   # (rows were actually dropped)


def test_evaluation_leaves_the_torch_generator_alone():
    nets = _nets()
    vec = _vec([_EpEnv(k, action_reward=True) for k in range(3)], nets, 4)
    state = torch.get_rng_state().clone()
    vec.run_evaluation(0)
    assert torch.equal(state, torch.get_rng_state())


def test_created_environments_are_seeded_seed_plus_i():
    sys.path.insert(0, os.path.join(ROOT, "tests", "envs"))
    from plugin import create_evaluator
    from synth_pendulum_data import env_creator  # noqa: F401  (the module create_env finds)
    from training.hip_trainer import HipEvaluator

    kw = dict(env_id="synth_pendulum", seed=5, num_eval_episode=3)
    ev = create_evaluator(hip_eval_env_num=3, networks=_nets(), **kw)
    one = HipEvaluator(networks=_nets(), **kw)
    first = lambda env: np.asarray(env.reset()[0])   # noqa: E731
    assert np.array_equal(first(ev.envs[0]), first(one.env))   # environment 0 is HipEvaluator's
    for i, env in enumerate(ev.envs[1:], 1):
        ref = create_evaluator(hip_eval_env_num=1, networks=_nets(), **dict(kw, seed=5 + i)).env
        assert np.array_equal(first(env), first(ref))


def test_header_prototype_matches_the_ffi_binding():
    import ctypes as C

    from dsact import _ffi

    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    m = re.search(r"int\s+dsact_act_mode_batch\s*\(([^)]*)\)\s*;", hdr)
    assert m, "dsact_act_mode_batch is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["dsact_handle* h", "const float* obs", "int32_t n", "float* action_host"], args
    entry = [s for s in _ffi.SYMBOLS if s[0] == "dsact_act_mode_batch"]
    assert len(entry) == 1
    _, res, argtypes = entry[0]
    assert res is C.c_int
    assert argtypes == [C.c_void_p, _ffi._FP, C.c_int32, _ffi._FP]
