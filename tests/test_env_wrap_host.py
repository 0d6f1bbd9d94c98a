"""The reference's environment wrappers on tensor environments (training/hip_tensor_env_wrappers.py) -- the
host side, without a GPU. Everything is compared BITWISE.

  1. the torch route on the CPU == tests/golden/env_wrap.npz, the reference's own wrapping_env recorded by
     scripts/env_wrap_golden.py (episodes terminated before the limit, truncated at it, and steps where both fire);
  2. lengths and flags == a Python-integer plan (tests/envs/synth_tensor_episodes_nolimit.py `plan`);
  3. an inner environment's own truncation is kept (OR); `elapsed` saturates;
  4. every refusal, the all-None identity, the state_dict round trip and its parameter check, attribute forwarding, the uint8
     pass-through;
  5. `hip_env_wrap` on HipTensorEnvSampler / HipTensorEnvEvaluator: routing, refusals, and bind_engine from the per-engine set-up;
  6. the two entry points are declared, exported and bound.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "dsac-v2_amd")
for _p in (ROOT, PKG, os.path.join(HERE, "envs")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_tensor_sampler_host import FakeEngine, _networks   # noqa: E402

M = 5
GOLDEN = os.path.join(HERE, "golden", "env_wrap.npz")


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint8 if a.dtype == np.bool_ else np.uint32 if a.dtype == np.float32 else a.dtype)


def _wrap(*args, **kw):
    from training.hip_tensor_env_wrappers import wrap_tensor_env

    return wrap_tensor_env(*args, **kw)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def test_torch_route_equals_the_reference_recording():
    from synth_tensor_episodes_nolimit import SynthTensorEpisodesNoLimit

    g = np.load(GOLDEN)
    R, T = g["reward"].shape
    assert (R, T) == (13, 40)
    # the recording holds all three kinds of episode end
    early = limit = both = 0
    for r in range(R):
        length = 0
        for s in range(T):
            length += 1
            if g["done"][r, s]:
                early += length < M and not g["truncated"][r, s]
                limit += length == M and bool(g["truncated"][r, s])
                both += length == M and not g["truncated"][r, s]
                assert length <= M
                length = 0
    assert early > 0 and limit > 0 and both > 0, (early, limit, both)
    env = _wrap(SynthTensorEpisodesNoLimit(R), max_episode_steps=M, reward_shift=0.3, reward_scale=0.7, obs_shift=0.1,
                obs_scale=g["obs_scale"])
    assert not env.fused
    obs = env.reset()
    for s in range(T):
        assert np.array_equal(_bits(obs), _bits(g["obs"][:, s])), s
        obs2, rew, term, trunc = env.step(torch.from_numpy(g["action"][:, s]))
        assert obs2.dtype == rew.dtype == torch.float32 and term.dtype == trunc.dtype == torch.bool
        assert np.array_equal(_bits(obs2), _bits(g["obs2"][:, s])), s
        assert np.array_equal(_bits(rew), _bits(g["reward"][:, s])), s
        assert np.array_equal((term | trunc).numpy(), g["done"][:, s]), s
        assert np.array_equal(trunc.numpy(), g["truncated"][:, s]), s
        obs = env.reset(term | trunc)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 5, 13, 20])
def test_lengths_and_flags_follow_the_integer_plan(limit):
    from synth_tensor_episodes_nolimit import SynthTensorEpisodesNoLimit, plan

    N = 16
    inner = SynthTensorEpisodesNoLimit(N)
    env = _wrap(inner, max_episode_steps=limit)
    assert env.reset() is not None and env.elapsed.dtype == torch.int32 and tuple(env.elapsed.shape) == (N,)
    where = env.elapsed.data_ptr()
    k, length = [0] * N, [0] * N
    act = torch.zeros(N, inner.act_dim)
    for _ in range(60):
        obs2, rew, term, trunc = env.step(act)
        for r in range(N):
            length[r] += 1
            want = plan(r, k[r], limit)
            ended = bool(term[r]) or bool(trunc[r])
            assert ended == (length[r] == want[0]), (r, k[r], length[r])
            if ended:
                assert (bool(term[r]), bool(trunc[r])) == want[1:], (r, k[r])
                k[r], length[r] = k[r] + 1, 0
        env.reset(term | trunc)
        assert env.elapsed.tolist() == length and env.elapsed.data_ptr() == where   # in place, zeroed where the mask is set
    assert min(k) >= 60 // 13


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_inner_truncation_is_kept_and_elapsed_saturates():
    from synth_tensor_episodes import SynthTensorEpisodes, limit_of

    N, limit = 12, 3
    bare, env = SynthTensorEpisodes(N), _wrap(SynthTensorEpisodes(N), max_episode_steps=limit)
    bare.reset()
    env.reset()
    act = torch.zeros(N, bare.act_dim)
    elapsed = [0] * N
    inner_only = outer_only = 0
    for _ in range(40):
        _, _, te, tr = bare.step(act)
        _, _, term, trunc = env.step(act)
        assert torch.equal(term, te)
        for r in range(N):
            elapsed[r] += 1
            hit = elapsed[r] >= limit
            assert bool(trunc[r]) == (bool(tr[r]) or (hit and not bool(te[r]))), r
            inner_only += bool(tr[r]) and not hit
            outer_only += hit and not bool(tr[r]) and not bool(te[r])
            if bool(term[r]) or bool(trunc[r]):
                elapsed[r] = 0
        ended = term | trunc
        bare.reset(ended)
        env.reset(ended)
    assert inner_only > 0 and outer_only > 0 and any(limit_of(r) < limit for r in range(N))
    # a row that is never reset stays at the limit
    env.reset()
    for _ in range(limit + 4):
        _, _, term, trunc = env.step(act)
    assert env.elapsed.tolist() == [limit] * N and torch.equal(trunc | term, torch.ones(N, dtype=torch.bool))
    big = _wrap(SynthTensorEpisodes(N), max_episode_steps=2 ** 31 - 2)     # the largest limit: elapsed + 1 still fits int32
    big.reset()
    big.elapsed.fill_(2 ** 31 - 3)
    for _ in range(3):
        _, _, term, trunc = big.step(act)
    assert big.elapsed.tolist() == [2 ** 31 - 2] * N and torch.equal(trunc | term, torch.ones(N, dtype=torch.bool))


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
class _Untouchable:
    """an environment no refusal may call"""
    num_envs, obs_dim = 4, 17

    def reset(self, mask=None):
        raise AssertionError("reset called")

    def step(self, action):
        raise AssertionError("step called")


@pytest.mark.parametrize("kw", [
    dict(max_episode_steps=0), dict(max_episode_steps=-3), dict(max_episode_steps=2.5), dict(max_episode_steps=5.0),
    dict(max_episode_steps=True), dict(max_episode_steps="5"), dict(max_episode_steps=2 ** 31 - 1),
    dict(reward_shift=float("nan")), dict(reward_scale=float("inf")), dict(reward_shift=[0.1, 0.2]),
    dict(obs_shift=float("-inf")), dict(obs_scale=[1.0] * 16 + [float("nan")]),
    dict(obs_scale=[1.0] * 16), dict(obs_shift=np.zeros((17, 1), np.float32)), dict(obs_shift=[0.0] * 17, obs_scale=[1.0] * 18),
])
def test_refusals_come_before_any_environment_call(kw):
    with pytest.raises(ValueError):
        _wrap(_Untouchable(), **kw)


def test_a_parameter_row_of_another_shape_than_the_first_rows_is_refused():
    from synth_tensor_humanoid import SynthTensorHumanoid

    env = _wrap(SynthTensorHumanoid(3), obs_scale=[1.0] * 17)     # (the environment names no row shape: known at reset())
    with pytest.raises(ValueError, match="obs_scale"):
        env.reset()


def test_all_none_is_the_environment_itself():
    env = _Untouchable()
    assert _wrap(env) is env and _wrap(env, None, None, None, None, None) is env


def test_parts_that_are_off_return_the_inner_tensors():
    from synth_tensor_episodes import SynthTensorEpisodes

    class Keep(SynthTensorEpisodes):
        def step(self, action):
            self.last = super().step(action)
            return self.last

    inner = Keep(4)
    env = _wrap(inner, max_episode_steps=3)
    env.reset()
    obs2, rew, term, trunc = env.step(torch.zeros(4, inner.act_dim))
    assert obs2 is inner.last[0] and rew is inner.last[1] and term is inner.last[2] and trunc is not inner.last[3]
    env = _wrap(Keep(4), reward_scale=0.5)       # the shift defaults to 0.0
    env.reset()
    obs2, rew, term, trunc = env.step(torch.zeros(4, inner.act_dim))
    assert obs2 is env.env.last[0] and term is env.env.last[2] and trunc is env.env.last[3]
    assert np.array_equal(_bits(rew), _bits((env.env.last[1] + 0.0) * 0.5))
    env = _wrap(Keep(4), obs_shift=0.25)         # the scale defaults to 1.0
    first = env.reset()
    obs2, rew, term, trunc = env.step(torch.zeros(4, inner.act_dim))
    assert rew is env.env.last[1] and np.array_equal(_bits(obs2), _bits((env.env.last[0] + 0.25) * 1.0))
    assert obs2.data_ptr() != first.data_ptr()   # step's obs2 and reset's obs live in different buffers
    again = env.reset(torch.zeros(4, dtype=torch.bool))
    assert again.data_ptr() == first.data_ptr() and np.array_equal(_bits(again), _bits(obs2))   # every row is scaled, none restarted


def test_state_dict_round_trip_and_parameter_check():
    from synth_tensor_humanoid import SynthTensorHumanoid
    from synth_tensor_humanoid_inplace import SynthTensorHumanoidInplace

    N = 6
    kw = dict(max_episode_steps=7, reward_shift=0.25, obs_scale=0.5)

    def make(**over):
        return _wrap(SynthTensorHumanoidInplace(N, seed=2, episode_limit=1000), **dict(kw, **over))

    def drive(env, steps, first):
        out = []
        for s in range(first, first + steps):
            act = 0.3 * torch.sin(torch.arange(N * 17, dtype=torch.float32).reshape(N, 17) + s)
            obs2, rew, term, trunc = env.step(act)
            out.append([t.clone() for t in (obs2, rew, term, trunc)])
            out.append([env.reset(term | trunc).clone()])
        return out

    a = make()
    a.reset()
    drive(a, 10, 0)                               # 10 steps: every row is 3 steps into its second episode (or restarted since)
    sd = a.state_dict()
    assert sorted(sd) == ["elapsed", "format", "inner", "params"] and sd["elapsed"].device.type == "cpu"
    assert 0 < int(sd["elapsed"].max()) < 7
    b = make()
    b.reset()
    where = b.elapsed.data_ptr()
    b.load_state_dict(sd)
    assert b.elapsed.data_ptr() == where and torch.equal(b.elapsed, a.elapsed)
    for x, y in zip(drive(a, 12, 10), drive(b, 12, 10)):
        for u, v in zip(x, y):
            assert np.array_equal(_bits(u), _bits(v))
    for over in (dict(max_episode_steps=8), dict(reward_shift=0.5), dict(obs_scale=0.25), dict(obs_shift=0.1)):
        c = make(**over)
        c.reset()
        with pytest.raises(ValueError, match="wrapped with"):
            c.load_state_dict(sd)
    with pytest.raises(ValueError, match="not a"):
        b.load_state_dict({"format": "other"})
    with pytest.raises(ValueError, match="elapsed"):
        b.load_state_dict(dict(sd, elapsed=sd["elapsed"] + 7))     # past the limit: never a value the wrapper wrote
    plain = _wrap(SynthTensorHumanoid(N, seed=2), **kw)      # no state_dict() of its own
    plain.reset()
    with pytest.raises(NotImplementedError, match="state_dict"):
        plain.state_dict()


def test_attributes_forward_to_the_inner_environment():
    from synth_tensor_episodes import SynthTensorEpisodes
    from synth_tensor_episodes_inplace import SynthTensorEpisodesInplace

    inner = SynthTensorEpisodesInplace(5)
    env = _wrap(inner, max_episode_steps=9)
    assert env.num_envs == 5 and env.action_low is inner.action_low and env.action_high is inner.action_high
    assert env.capture_safe is True and env.obs_dim == 17 and env.env is inner and env.max_episode_steps == 9
    plain = _wrap(SynthTensorEpisodes(5), reward_shift=1.0)
    assert getattr(plain, "capture_safe", False) is False and not hasattr(plain, "max_episode_steps")
    inner.max_episode_steps = 123                 # the inner attribute is forwarded, never taken as the wrapper's limit
    shaped = _wrap(inner, reward_shift=1.0)
    assert shaped.max_episode_steps == 123 and shaped._limit is None
    with pytest.raises(AttributeError):
        env.no_such_attribute


def test_uint8_frames_pass_through_untouched():
    from synth_tensor_blob import SynthTensorBlob

    class Keep(SynthTensorBlob):
        def reset(self, mask=None):
            self.last = super().reset(mask)
            return self.last

        def step(self, action):
            self.last_step = super().step(action)
            return self.last_step

    inner = Keep(2, frames="uint8")
    env = _wrap(inner, max_episode_steps=3, reward_shift=0.5)
    assert env.reset() is inner.last and inner.last.dtype == torch.uint8
    for s in range(3):
        obs2, rew, term, trunc = env.step(torch.zeros(2, 3))
        assert obs2 is inner.last_step[0] and term is inner.last_step[2]
        assert np.array_equal(_bits(rew), _bits((inner.last_step[1] + 0.5) * 1.0))
        assert trunc.tolist() == [s == 2] * 2
        assert env.reset(term | trunc) is inner.last
    with pytest.raises(NotImplementedError, match="uint8"):
        _wrap(Keep(2, frames="uint8"), obs_scale=2.0).reset()
    # float32 frames take a [C, H, W] parameter
    ramp = np.linspace(0.5, 1.5, 3 * 96 * 96).astype(np.float32).reshape(3, 96, 96)
    frames = _wrap(Keep(2), obs_shift=-0.5, obs_scale=ramp)
    got = frames.reset()
    assert np.array_equal(_bits(got), _bits((frames.env.last + (-0.5)) * torch.from_numpy(ramp)))


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
class WrapEngine(FakeEngine):
    """FakeEngine with the two wrapper calls restated in torch ops: what the fused route hands to the engine"""

    def act_mode_device(self, obs, action):
        action.zero_()

    def env_wrap_step(self, n, obs2=None, rew=None, terminated=None, truncated=None, obs_shift=None, obs_scale=None, reward_shift=0.0,
                      reward_scale=1.0, reward_on=False, max_episode_steps=0, elapsed=None, obs2_out=None, rew_out=None,
                      truncated_out=None):
        self.calls.append(("env_wrap_step", n, obs2_out is not None, bool(reward_on), int(max_episode_steps)))
        if obs2_out is not None:
            obs2_out.copy_((obs2 + obs_shift.view(obs2.shape[1:])) * obs_scale.view(obs2.shape[1:]))
        if reward_on:
            rew_out.copy_((rew + float(reward_shift)) * float(reward_scale))
        if max_episode_steps:
            elapsed.copy_(torch.clamp(elapsed + 1, max=max_episode_steps))
            truncated_out.copy_(truncated | ((elapsed >= max_episode_steps) & ~terminated))

    def env_wrap_reset(self, n, obs=None, mask=None, obs_shift=None, obs_scale=None, elapsed=None, obs_out=None):
        self.calls.append(("env_wrap_reset", n, obs_out is not None, elapsed is not None, mask is not None))
        if obs_out is not None:
            obs_out.copy_((obs + obs_shift.view(obs.shape[1:])) * obs_scale.view(obs.shape[1:]))
        if elapsed is not None:
            if mask is None:
                elapsed.zero_()
            else:
                elapsed.masked_fill_(mask, 0)


def _wrapped_sampler(eng, N=4, S=8, **over):
    from plugin import create_sampler
    from synth_tensor_episodes_nolimit import SynthTensorEpisodesNoLimit

    inner = SynthTensorEpisodesNoLimit(N)
    kw = dict(sampler_name="hip_tensor_env_sampler", env=inner, sample_batch_size=S, networks=_networks(eng), seed=3)
    return create_sampler(**dict(kw, **over)), inner


def test_hip_env_wrap_on_the_sampler():
    from training.hip_tensor_env_wrappers import WrappedTensorEnv

    eng = FakeEngine(obs_dim=17, act_dim=6)
    smp, inner = _wrapped_sampler(eng, max_episode_steps=5, reward_shift=0.3, reward_scale=0.7)
    assert smp.env is inner                                        # the default is off: the environment as it came
    smp, inner = _wrapped_sampler(eng, hip_env_wrap=False, max_episode_steps=5)
    assert smp.env is inner
    ramp = np.linspace(0.5, 1.5, 17).astype(np.float32)
    eng = WrapEngine(obs_dim=17, act_dim=6)
    smp, inner = _wrapped_sampler(eng, hip_env_wrap=True, max_episode_steps=5, reward_shift=0.3, reward_scale=0.7, obs_shift=0.1,
                                  obs_scale=ramp)
    env = smp.env
    assert isinstance(env, WrappedTensorEnv) and env.env is inner and smp.reward_scale == 0.7
    assert env._limit == 5 and env._reward == (np.float32(0.3), np.float32(1.0))      # reward_scale stays with the ring write
    assert np.array_equal(env._obs_params[0], np.float32(0.1)) and np.array_equal(env._obs_params[1], ramp)
    assert not env.fused
    batch, _ = smp.sample()                       # _setup binds the engine behind the first reset(): one call per step and reset
    assert env.fused and env._engine is eng
    wraps = [c for c in eng.calls if c[0].startswith("env_wrap")]
    assert wraps == [("env_wrap_step", 4, True, True, 5), ("env_wrap_reset", 4, True, True, True)] * 2
    # ... and computes what the torch route computes
    ref_eng = FakeEngine(obs_dim=17, act_dim=6)
    ref, _ = _wrapped_sampler(ref_eng, hip_env_wrap=True, max_episode_steps=5, reward_shift=0.3, reward_scale=0.7, obs_shift=0.1,
                              obs_scale=ramp)
    ref.env.use_fused = False                                      # (FakeEngine has no wrapper calls: any would raise)
    want, _ = ref.sample()
    assert not ref.env.fused
    for u, v in zip(batch.device_columns, want.device_columns):
        assert np.array_equal(_bits(u), _bits(v))
    # only some of the four set
    smp, inner = _wrapped_sampler(FakeEngine(obs_dim=17, act_dim=6), hip_env_wrap=True, obs_scale=2.0)
    assert smp.env._limit is None and smp.env._reward is None and smp.env._obs_params[1] == np.float32(2.0)
    for bad in ("yes", 1, None, 0):
        with pytest.raises(ValueError, match="hip_env_wrap must be"):
            _wrapped_sampler(eng, hip_env_wrap=bad, max_episode_steps=5)
    with pytest.raises(ValueError, match="does nothing"):
        _wrapped_sampler(eng, hip_env_wrap=True, reward_scale=0.7)  # reward_scale alone is not the wrapper's
    with pytest.raises(ValueError, match="max_episode_steps"):
        _wrapped_sampler(eng, hip_env_wrap=True, max_episode_steps=0)


def test_hip_env_wrap_on_the_evaluator():
    from plugin import create_evaluator
    from synth_tensor_episodes_nolimit import SynthTensorEpisodesNoLimit, plan
    from training.hip_tensor_env_wrappers import WrappedTensorEnv

    N, E = 4, 8

    class EvalEngine(WrapEngine):
        """WrapEngine with the evaluation bookkeeping in Python"""

        def eval_begin(self, n, e):
            self.ep, self.acc, self.len = list(range(n)), [0.0] * n, [0] * n
            self.returns, self.lengths, self.e = [0.0] * e, [0] * e, e

        def eval_commit(self, rew, term, trunc, ended):
            ended.copy_(term | trunc)
            for i in range(len(self.ep)):
                if self.ep[i] < self.e:
                    self.acc[i] += float(rew[i])
                    self.len[i] += 1
                    if bool(ended[i]):
                        self.returns[self.ep[i]], self.lengths[self.ep[i]] = self.acc[i], self.len[i]
                        self.ep[i], self.acc[i], self.len[i] = self.ep[i] + len(self.ep), 0.0, 0

        def eval_poll(self):
            return sum(1 for x in self.lengths if x == 0)

        def eval_read(self, e):
            return np.array(self.returns, np.float64), np.array(self.lengths, np.int32)

        def note_torch_writes(self, params):
            pass

    def make(eng, **over):
        inner = SynthTensorEpisodesNoLimit(N)
        kw = dict(evaluator_name="hip_tensor_env_evaluator", eval_env=inner, num_eval_episode=E, networks=_networks(eng))
        return create_evaluator(**dict(kw, **over)), inner

    ev, inner = make(EvalEngine(obs_dim=17, act_dim=6), max_episode_steps=5)
    assert ev.env is inner
    eng = EvalEngine(obs_dim=17, act_dim=6)
    ev, inner = make(eng, hip_env_wrap=True, max_episode_steps=5, reward_shift=0.3, reward_scale=0.7)
    assert isinstance(ev.env, WrappedTensorEnv) and ev.env._limit == 5
    assert ev.env._reward == (np.float32(0.3), np.float32(1.0))     # the shift is passed, the scale is not
    ev.run_evaluation(0)
    assert ev.env.fused and any(c[0] == "env_wrap_step" for c in eng.calls)
    assert ev.lengths.tolist() == [plan(e % N, e // N, 5)[0] for e in range(E)]
    # eval_save without hip_eval_save_max_steps takes the wrapper's max_episode_steps (the bare fixture has none)
    with pytest.raises(ValueError, match="hip_eval_save_max_steps"):
        make(eng, eval_save=True, save_folder="unused")
    ev, _ = make(eng, eval_save=True, save_folder="unused", hip_env_wrap=True, max_episode_steps=5)
    assert ev.save_max_steps == 5
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="hip_env_wrap must be"):
            make(eng, hip_env_wrap=bad, max_episode_steps=5)
    with pytest.raises(ValueError, match="does nothing"):
        make(eng, hip_env_wrap=True)


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    import ctypes as C

    from dsact import _ffi

    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    P = C.c_void_p
    want = {
        "dsact_env_wrap_step": (r"int dsact_env_wrap_step\(dsact_handle\* h, int32_t n, int32_t row_floats, const float\* obs2_dev, "
                                r"const float\* rew_dev,\s+const uint8_t\* terminated_dev, const uint8_t\* truncated_dev, "
                                r"const float\* obs_shift_dev,\s+const float\* obs_scale_dev, float reward_shift, float reward_scale, "
                                r"int32_t reward_on,\s+int32_t max_episode_steps, int32_t\* elapsed_dev, float\* obs2_out, "
                                r"float\* rew_out, uint8_t\* truncated_out\);",
                                [P, C.c_int32, C.c_int32, P, P, P, P, P, P, C.c_float, C.c_float, C.c_int32, C.c_int32, P, P, P, P]),
        "dsact_env_wrap_reset": (r"int dsact_env_wrap_reset\(dsact_handle\* h, int32_t n, int32_t row_floats, const float\* obs_dev, "
                                 r"const uint8_t\* mask_dev,\s+const float\* obs_shift_dev, const float\* obs_scale_dev, "
                                 r"int32_t\* elapsed_dev, float\* obs_out\);", [P, C.c_int32, C.c_int32, P, P, P, P, P, P]),
    }
    bound = {n: (res, args) for n, res, args in _ffi.SYMBOLS}
    for name, (decl, args) in want.items():
        assert re.search(decl, hdr), name
        assert bound[name] == (C.c_int, args), name
    assert '"env_wrap_calls"' in hdr
    lib = _ffi.load()
    for name in want:
        assert hasattr(lib, name), name
    # without a handle the entry points refuse like every other one
    assert lib.dsact_env_wrap_step(None, 1, 0, None, None, None, None, None, None, 0.0, 1.0, 1, 0, None, None, None, None) == -1
    assert lib.dsact_env_wrap_reset(None, 1, 0, None, None, None, None, None, None) == -1
