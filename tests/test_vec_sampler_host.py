"""HipVecOffSampler (training/hip_vec_sampler.py) on CPU: unattached containers act through the module forward, so the
lockstep loop, its transition order and its per-environment semantics are checked here without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))


class _Box:
    def __init__(self, lim, n):
        self.low, self.high = np.full(n, -lim, np.float32), np.full(n, lim, np.float32)


class _VarEnv:
    """deterministic dynamics whose episodes end at different steps per environment: environment k is truncated after 3 + k
    steps and, every other episode, environment 2 terminates after 2 steps"""
    O, A = 5, 2

    def __init__(self, k):
        self.k, self.t, self.ep = k, 0, 0
        self.action_space = _Box(0.3, self.A)
        self.s = np.zeros(self.O, np.float32)

    def reset(self):
        self.t, self.ep = 0, self.ep + 1
        self.s = np.linspace(-1, 1, self.O).astype(np.float32) * (1 + 0.1 * self.k)
        return self.s.copy(), {"ep": self.ep}

    def step(self, a):
        self.t += 1
        self.s = (0.9 * self.s + 0.2 * np.resize(a, self.O)).astype(np.float32)
        term = self.k == 2 and self.ep % 2 == 1 and self.t == 2
        return self.s.copy(), float(self.s.sum()), term, {"TimeLimit.truncated": self.t >= 3 + self.k}


def _nets(O, A, lim, seed=0):
    from dsac_v2_hip import ApproxContainer

    torch.manual_seed(seed)
    return ApproxContainer(**hip_kwargs(O, A, (32, 32), 16, act_limit=lim))


def _reference_loop(envs, nets, steps, scale=1.0):
    """one environment at a time, in the sampler's order, acting row by row with the rows of ONE torch.randn(N, A) draw
    per step; returns the transitions step-major"""
    N = len(envs)
    state = []
    for e in envs:
        o, i = e.reset()
        state.append([np.asarray(o, np.float32), i])
    out = []
    for _ in range(steps):
        A = envs[0].action_space.low.shape[0]
        eps = torch.randn(N, A)
        for i, e in enumerate(envs):
            obs, info = state[i]
            with torch.no_grad():
                logits = nets.policy(torch.from_numpy(obs.reshape(1, -1)))
                dist = nets.create_action_distributions(logits)
                act, lp = dist._squash(dist.mean + eps[i:i + 1] * dist.std)
            act = act[0].numpy()
            clipped = np.clip(act, e.action_space.low, e.action_space.high)
            o2, r, done, ni = e.step(clipped)
            tr = bool(ni.get("TimeLimit.truncated", False))
            done = bool(done) and not tr
            out.append((obs, info, act, scale * r, np.asarray(o2, np.float32), done, float(lp[0]), tr))
            state[i] = [np.asarray(o2, np.float32), ni]
            if done or tr:
                o, inf = e.reset()
                state[i] = [np.asarray(o, np.float32), inf]
    return out


def _check_against(batch, ref, atol=1e-5):
    assert len(batch) == len(ref)
    obs_b, act_b, rew_b, obs2_b, done_b, logp_b = batch.packed
    for j, (s, r) in enumerate(zip(batch, ref)):
        np.testing.assert_allclose(np.reshape(s[0], -1), r[0], atol=atol, rtol=0)
        assert s[1] == r[1]
        np.testing.assert_allclose(s[2], r[2], atol=atol, rtol=0)
        assert abs(s[3] - r[3]) <= 1e-4 * max(1.0, abs(r[3]))
        np.testing.assert_allclose(np.reshape(s[4], -1), r[4], atol=atol, rtol=0)
        assert s[5] == r[5] and s[7]["TimeLimit.truncated"] == r[7]
        assert abs(float(s[6]) - r[6]) <= 1e-4 * max(1.0, abs(r[6]))
        # packed == the tuples, row for row
        assert np.array_equal(obs_b[j], np.reshape(s[0], -1)) and np.array_equal(obs2_b[j], np.reshape(s[4], -1))
        assert np.array_equal(act_b[j], s[2]) and rew_b[j] == np.float32(s[3])
        assert done_b[j] == float(s[5]) and logp_b[j] == np.float32(s[6])


def test_n1_is_hip_off_sampler_bitwise():
    from plugin import create_sampler
    from training.hip_sampler import HipOffSampler

    kw = hip_kwargs(3, 1, (32, 32), 16, act_limit=2.0, env_id="synth_pendulum", sample_batch_size=20, seed=3)
    runs = []
    for make in (lambda: HipOffSampler(**kw), lambda: create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=1, **kw)):
        torch.manual_seed(0)
        smp = make()
        torch.manual_seed(1)
        batches = [smp.sample()[0] for _ in range(12)]    # 240 steps: the 200-step time limit resets once
        runs.append((batches, torch.randn(3), smp.get_total_sample_number()))
    (b0, r0, n0), (b1, r1, n1) = runs
    assert torch.equal(r0, r1) and n0 == n1 == 240
    for x, y in zip(b0, b1):
        assert len(x) == len(y)
        for s, t in zip(x, y):
            assert np.array_equal(s[0], t[0]) and np.array_equal(s[2], t[2]) and np.array_equal(s[4], t[4])
            assert s[3] == t[3] and s[5] == t[5] and np.array_equal(s[6], t[6]) and s[7] == t[7]


def test_n3_matches_per_environment_loop_with_independent_resets():
    from training.hip_vec_sampler import HipVecOffSampler

    nets = _nets(_VarEnv.O, _VarEnv.A, 0.3)
    smp = HipVecOffSampler(envs=[_VarEnv(k) for k in range(3)], networks=nets, sample_batch_size=12, action_type="continu",
                           reward_scale=0.5)
    assert smp.route() == "module"
    torch.manual_seed(5)
    batches = [smp.sample()[0] for _ in range(4)]    # 16 lockstep steps
    after = torch.randn(2)
    torch.manual_seed(5)
    ref = _reference_loop([_VarEnv(k) for k in range(3)], nets, 16, scale=0.5)
    assert torch.equal(after, torch.randn(2))          # the generator was consumed the same
    for b in range(4):
        _check_against(batches[b], ref[12 * b:12 * (b + 1)])
    # the episodes ended at different steps and each environment was reset on its own
    flat = [s for b in batches for s in b]
    for k in range(3):
        rows = flat[k::3]
        ends = [t for t, s in enumerate(rows) if s[5] or s[7]["TimeLimit.truncated"]]
        assert ends and ends[0] in (1, 2 + k)
    assert any(s[5] for s in flat[2::3]) and not any(s[5] for s in flat[0::3])
    assert all(s[7]["TimeLimit.truncated"] is False for s in flat if s[5])


def test_n3_synth_humanoid_seeds_and_step_major_order():
    from plugin import create_sampler
    from synth_humanoid_data import SynthHumanoid

    kw = hip_kwargs(376, 17, (32, 32), 16, act_limit=0.4, env_id="synth_humanoid", sample_batch_size=9, seed=11)
    torch.manual_seed(0)
    smp = create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=3, **kw)
    torch.manual_seed(0)
    nets = _nets(376, 17, 0.4)      # the throw-away container came from the same generator state
    for p, q in zip(smp.networks.parameters(), nets.parameters()):
        assert torch.equal(p, q)
    torch.manual_seed(2)
    batch, _ = smp.sample()
    envs = [SynthHumanoid(seed=11 + k) for k in range(3)]      # environment k seeded seed + k
    torch.manual_seed(2)
    _check_against(batch, _reference_loop(envs, nets, 3))


def test_truncation_stored_non_terminal():
    from training.hip_vec_sampler import HipVecOffSampler
    from test_hip_groups import _ToyEnv

    nets = _nets(16, 4, 0.3)
    smp = HipVecOffSampler(envs=[_ToyEnv() for _ in range(2)], networks=nets, sample_batch_size=16, action_type="continu")
    torch.manual_seed(3)
    batch, _ = smp.sample()
    assert [s[7]["TimeLimit.truncated"] for s in batch[:16:2]] == [False] * 6 + [True, False]
    assert not any(s[5] for s in batch) and not batch.packed[4].any()
    # after the time-out both environments started again from reset()'s state
    np.testing.assert_array_equal(batch[14][0], _ToyEnv().reset()[0])
    np.testing.assert_array_equal(batch[15][0], _ToyEnv().reset()[0])


def test_batch_size_must_be_a_multiple_of_n():
    from plugin import create_sampler

    kw = hip_kwargs(376, 17, (32, 32), 16, env_id="synth_humanoid", sample_batch_size=10, seed=0)
    with pytest.raises(ValueError, match="multiple"):
        create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=4, **kw)
    with pytest.raises(ValueError, match="multiple"):
        create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=3, batch_size_per_sampler=8,
                       **{k: v for k, v in kw.items() if k != "sample_batch_size"})
    with pytest.raises(ValueError):
        create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=2, envs=[object()] * 3, **kw)


def test_create_sampler_dispatch_and_unchanged_default():
    from plugin import create_sampler
    from training.hip_sampler import HipOffSampler
    from training.hip_vec_sampler import HipVecOffSampler

    kw = hip_kwargs(376, 17, (32, 32), 16, env_id="synth_humanoid", sample_batch_size=8, seed=0)
    vec = create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=4, **kw)
    assert type(vec) is HipVecOffSampler and vec.n_envs == 4 and len(vec.envs) == 4
    for extra in ({}, {"vector_env_num": 4}, {"sampler_name": "off_sampler", "vector_env_num": 4, "vector_env_type": "async"}):
        assert type(create_sampler(**kw, **extra)) is HipOffSampler


def test_trainer_loop_on_the_vectorised_sampler(tmp_path):
    from plugin import create_evaluator, create_sampler, create_trainer
    from test_trainer_host import HostBuffer, StubAlg

    kw = hip_kwargs(3, 1, (32, 32), 16, act_limit=2.0, env_id="synth_pendulum", sample_batch_size=20,
                    reward_scale=1, buffer_warm_size=100, max_iteration=12, log_save_interval=4,
                    apprfunc_save_interval=6, eval_interval=6, num_eval_episode=1, ini_network_dir=None,
                    save_folder=str(tmp_path), seed=3, sampler_name="hip_vec_off_sampler", vector_env_num=4)
    torch.manual_seed(0)
    sampler = create_sampler(**kw)
    from dsac_v2_hip import ApproxContainer

    nets = ApproxContainer(**kw)
    alg = StubAlg(nets)
    buf = HostBuffer(3, 1, 1000)
    trainer = create_trainer(alg, sampler, buf, create_evaluator(**kw), **kw)
    assert sampler.networks is nets and buf.size >= 100
    trainer.train()
    assert alg.calls == list(range(12))
    assert sampler.get_total_sample_number() == buf.size


def test_n1_wrapping_sample_does_not_recurse():
    """a caller that wraps sampler.sample (a timing loop) wraps the vectorised sampler's method, not the inner sampler's"""
    from plugin import create_sampler

    kw = hip_kwargs(3, 1, (32, 32), 16, act_limit=2.0, env_id="synth_pendulum", sample_batch_size=4, seed=3)
    smp = create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=1, **kw)
    inner, calls = smp.sample, []
    smp.sample = lambda: calls.append(1) or inner()
    assert len(smp.sample()[0]) == 4 and calls == [1] and smp.get_total_sample_number() == 4
