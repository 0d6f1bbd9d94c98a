"""A sample() as one captured graph (training/hip_tensor_sampler.py with hip_graph_sample=True) -- the host
side, without a GPU.

  1. the five entry points (dsact_act_counter_set / _add / _read, dsact_act_sample_device_counted, dsact_step_rows_device) are
     declared, exported and bound alike;
  2. the constructor's refusals come before the environment is reset or stepped and before the engine is called; an engine off
     the GPU is refused at the first sample(); without the kwarg the sampler makes the calls it always made;
  3. tests/envs/synth_tensor_humanoid_inplace.py equals tests/envs/synth_tensor_humanoid.py bit for bit, in the sampler's own
     step / reset(mask) order, with terminations and truncations on the way;
  4. its state tensors keep their storage.
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

O, A = 376, 17


# ---- 1. the C-ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    import ctypes as C

    from dsact import _ffi

    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    P = C.c_void_p
    want = {
        "dsact_act_counter_set": (r"int dsact_act_counter_set\(dsact_handle\* h, uint64_t step\);", [P, C.c_uint64]),
        "dsact_act_counter_add": (r"int dsact_act_counter_add\(dsact_handle\* h, int64_t k\);", [P, C.c_int64]),
        "dsact_act_counter_read": (r"int dsact_act_counter_read\(dsact_handle\* h, uint64_t\* out\);", [P, C.POINTER(C.c_uint64)]),
        "dsact_act_sample_device_counted": (r"int dsact_act_sample_device_counted\(dsact_handle\* h, const float\* obs_dev, int32_t n, "
                                            r"int64_t step_offset, float\* action_dev,\s+float\* clipped_dev, float\* logp_dev\);",
                                            [P, P, C.c_int32, C.c_int64, P, P, P]),
        "dsact_step_rows_device": (r"int dsact_step_rows_device\(dsact_handle\* h, int32_t n, int32_t row_floats, const float\* obs2_dev, "
                                   r"const float\* rew_dev,\s+const uint8_t\* terminated_dev, const uint8_t\* truncated_dev, "
                                   r"float\* obs2_slot, float\* rew_slot,\s+uint8_t\* terminated_slot, uint8_t\* truncated_slot, "
                                   r"uint8_t\* ended_dev\);",
                                   [P, C.c_int32, C.c_int32, P, P, P, P, P, P, P, P, P]),
    }
    bound = {n: (res, args) for n, res, args in _ffi.SYMBOLS}
    for name, (decl, args) in want.items():
        assert re.search(decl, hdr), name
        assert bound[name] == (C.c_int, args), name
    doc = hdr[hdr.index("A sample() as one captured graph"):hdr.index("int dsact_act_counter_set")]
    for word in ("off_sampler.py:46-84", "off_sampler.py:66-84", "DSACT_E_STATE under stream capture", "carry included",
                 "LEGAL WHILE THE HANDLE'S STREAM IS CAPTURING"):
        assert word in doc, word
    lib = _ffi.load()
    for name in want:
        assert hasattr(lib, name), name
    # without a handle the entry points refuse like every other one
    assert lib.dsact_act_counter_set(None, 1) == -1
    assert lib.dsact_act_counter_add(None, 1) == -1
    assert lib.dsact_act_counter_read(None, None) == -1
    assert lib.dsact_act_sample_device_counted(None, None, 1, 0, None, None, None) == -1
    assert lib.dsact_step_rows_device(None, 1, 1, None, None, None, None, None, None, None, None, None) == -1
    # the engine offers each under its own name
    from dsact.engine import DsactEngine
    for name in ("act_counter_set", "act_counter_add", "act_counter_read", "act_sample_device_counted", "step_rows_device"):
        assert callable(getattr(DsactEngine, name)), name


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
class RecordingEnv:
    """speaks the protocol's attributes and records every reset / step: a refusal must come before either"""
    num_envs = 8

    def __init__(self, **attrs):
        self.action_low, self.action_high = torch.full((A,), -0.4), torch.full((A,), 0.4)
        self.calls = []
        for k, v in attrs.items():
            setattr(self, k, v)

    def reset(self, mask=None):
        self.calls.append("reset")
        return torch.zeros(self.num_envs, O)

    def step(self, action):
        self.calls.append("step")
        z = torch.zeros(self.num_envs)
        return torch.zeros(self.num_envs, O), z, z > 1, z > 1


def _create(env, eng, **over):
    from plugin import create_sampler
    return create_sampler(sampler_name="hip_tensor_env_sampler", env=env, sample_batch_size=16, networks=_networks(eng), seed=3, **over)


def test_refusals_come_before_any_environment_or_engine_call():
    for attrs in ({}, {"capture_safe": False}, {"capture_safe": 1}):      # absent, False, and truthy-but-not-True
        env, eng = RecordingEnv(**attrs), FakeEngine()
        with pytest.raises(NotImplementedError, match="capture_safe"):
            _create(env, eng, hip_graph_sample=True)
        assert env.calls == [] and eng.calls == []
    env, eng = RecordingEnv(capture_safe=True), FakeEngine()
    with pytest.raises(NotImplementedError, match="hip_cnn_act"):
        _create(env, eng, hip_graph_sample=True, hip_cnn_act=True)
    assert env.calls == [] and eng.calls == []
    for bad in (1, 0, "yes", None, 1.0):
        env, eng = RecordingEnv(capture_safe=True), FakeEngine()
        with pytest.raises(ValueError, match="hip_graph_sample"):
            _create(env, eng, hip_graph_sample=bad)
        assert env.calls == [] and eng.calls == []


def test_an_engine_off_the_gpu_is_refused_at_the_first_sample():
    env, eng = RecordingEnv(capture_safe=True), FakeEngine()
    smp = _create(env, eng, hip_graph_sample=True)                     # the constructor cannot know the engine's device yet
    assert smp.graph_sample and smp.graph_captures == 0 and smp.graph_replays == 0
    assert env.calls == [] and eng.calls == []
    with pytest.raises(NotImplementedError, match="GPU"):
        smp.sample()
    assert env.calls == [] and eng.calls == []
    assert smp.graph_captures == 0 and smp.graph_replays == 0 and smp.act_step == 0


def test_without_the_kwarg_the_sampler_makes_the_calls_it_always_made():
    """act_step became a property; the eager route neither knows the device counter nor the one-launch row copies"""
    for over in ({}, {"hip_graph_sample": False}):
        env, eng = RecordingEnv(capture_safe=True), FakeEngine()
        smp = _create(env, eng, **over)
        assert not smp.graph_sample
        smp.sample()
        smp.act_step = 1000
        smp.sample()
        names = [c[0] for c in eng.calls]
        assert names == ["set_act_rng"] + ["act_sample_device"] * 4
        assert [c[2] for c in eng.calls[1:]] == [0, 1, 1000, 1001] and smp.act_step == 1002
        assert smp.graph_captures == 0 and smp.graph_replays == 0


# ---- 3. / 4. the in-place fixture ----------------------------------------------------------------------------------------------------
def _walk(env, actions):
    """the sampler's own order: reset(), then per step step(a) and reset(terminated | truncated); everything it returns, cloned"""
    out = [env.reset().clone()]
    for a in actions:
        obs2, rew, term, trunc = env.step(a)
        out.append((obs2.clone(), rew.clone(), term.clone(), trunc.clone(), env.pos.clone(), env.t.clone()))
        nxt = env.reset(term | trunc)
        out.append((nxt.clone(), env.pos.clone(), env.t.clone()))
    return out


def test_the_inplace_fixture_equals_the_plain_one_bit_for_bit():
    from synth_tensor_humanoid import SynthTensorHumanoid
    from synth_tensor_humanoid_inplace import SynthTensorHumanoidInplace

    N, steps, seed = 8, 64, 4
    limit = torch.arange(3, 3 + N)                                      # 3 .. 10: every environment times out, at its own pace
    g = torch.Generator().manual_seed(11)
    actions = [0.8 * torch.rand(N, A, generator=g) - 0.4 for _ in range(steps)]
    plain = SynthTensorHumanoid(N, seed=seed, episode_limit=limit)
    inpl = SynthTensorHumanoidInplace(N, seed=seed, episode_limit=limit)
    assert inpl.capture_safe is True and getattr(plain, "capture_safe", False) is not True
    a, b = _walk(plain, actions), _walk(inpl, actions)
    assert torch.equal(a[0], b[0])
    n_term = n_trunc = 0
    for k, (x, y) in enumerate(zip(a[1:], b[1:])):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert u.dtype == v.dtype and torch.equal(u, v), k
        if len(x) == 6:
            n_term += int(x[2].sum())
            n_trunc += int(x[3].sum())
    assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)              # both kinds of episode end were on the way
    assert torch.equal(plain.pos, inpl.pos) and torch.equal(plain.t, inpl.t)


def test_the_inplace_fixture_keeps_its_state_tensors():
    from synth_tensor_humanoid_inplace import SynthTensorHumanoidInplace

    N = 8
    env = SynthTensorHumanoidInplace(N, seed=4, episode_limit=torch.arange(3, 3 + N))
    ptrs = (env.pos.data_ptr(), env.t.data_ptr())
    pos, t = env.pos, env.t
    g = torch.Generator().manual_seed(5)
    env.reset()
    assert (env.pos.data_ptr(), env.t.data_ptr()) == ptrs
    ended = 0
    for _ in range(16):
        _, _, term, trunc = env.step(0.8 * torch.rand(N, A, generator=g) - 0.4)
        assert (env.pos.data_ptr(), env.t.data_ptr()) == ptrs and env.pos is pos and env.t is t
        ended += int((term | trunc).sum())
        env.reset(term | trunc)
        assert (env.pos.data_ptr(), env.t.data_ptr()) == ptrs and env.pos is pos and env.t is t
    assert ended >= 8
    sd = env.state_dict()
    env.step(torch.zeros(N, A))
    env.load_state_dict(sd)
    assert (env.pos.data_ptr(), env.t.data_ptr()) == ptrs and torch.equal(env.pos, sd["pos"]) and torch.equal(env.t, sd["t"])
