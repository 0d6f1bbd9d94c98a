"""Image tensor environments inside the sample / eval graphs -- the host side, without a GPU:

  1. the three entry points (dsact_cnn_acting_capture, dsact_act_sample_device_counted_u8, dsact_step_frames_device) are declared,
     exported and bound alike;
  2. `hip_graph_sample=True` / `hip_graph_eval=True` with `hip_cnn_act=True` is accepted on an image engine with the CNN acting
     path and refused on every other engine before any environment or engine call -- in the constructor, or at the first call
     for a policy attached later;
  3. the engine's opt-in (cnn_acting_capture) is made once per engine and only on the graph route; without the kwargs the call
     sequence is the one it always was; the row move of a step is one step_frames_device for contiguous image rows, the torch
     copies otherwise;
  4. tests/envs/synth_tensor_blob_inplace.py equals tests/envs/synth_tensor_blob.py bit for bit in both frame dtypes, and its
     state tensors keep their storage.

A graph is captured from a GPU stream, so what runs here is the route's first call on an engine: the eager warm-up, which issues
exactly the body that the capture records (the device check is stepped over: require_graph_device).
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

from test_tensor_image_host import FakeCnnEngine   # noqa: E402
from test_tensor_sampler_host import FakeEngine, _networks   # noqa: E402

SHAPE, A = (3, 96, 96), 3


# ---- 1. the C-ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    import ctypes as C

    from dsact import _ffi

    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    P = C.c_void_p
    want = {
        "dsact_cnn_acting_capture": (r"int dsact_cnn_acting_capture\(dsact_handle\* h, int32_t on\);", [P, C.c_int32]),
        "dsact_act_sample_device_counted_u8": (r"int dsact_act_sample_device_counted_u8\(dsact_handle\* h, const uint8_t\* frames_dev, "
                                               r"int32_t n, int64_t step_offset, float\* action_dev,\s+float\* clipped_dev, "
                                               r"float\* logp_dev\);", [P, P, C.c_int32, C.c_int64, P, P, P]),
        "dsact_step_frames_device": (r"int dsact_step_frames_device\(dsact_handle\* h, int32_t n, int64_t row_bytes, const void\* obs2_dev, "
                                     r"const float\* rew_dev,\s+const uint8_t\* terminated_dev, const uint8_t\* truncated_dev, "
                                     r"void\* obs2_slot, float\* rew_slot,\s+uint8_t\* terminated_slot, uint8_t\* truncated_slot, "
                                     r"uint8_t\* ended_dev\);", [P, C.c_int32, C.c_int64, P, P, P, P, P, P, P, P, P]),
    }
    bound = {n: (res, args) for n, res, args in _ffi.SYMBOLS}
    for name, (decl, args) in want.items():
        assert re.search(decl, hdr), name
        assert bound[name] == (C.c_int, args), name
    doc = hdr[hdr.index("Image environments inside sample / eval graphs"):hdr.index("int dsact_cnn_acting_capture")]
    for word in ("WHY OPT-IN", "behind EVERYTHING enqueued", "STICKY", "one linear chain", "cnn_act_capture", "step_frames_calls"):
        assert word in doc, word
    lib = _ffi.load()
    for name in want:
        assert hasattr(lib, name), name
    assert lib.dsact_cnn_acting_capture(None, 1) == -1
    assert lib.dsact_act_sample_device_counted_u8(None, None, 1, 0, None, None, None) == -1
    assert lib.dsact_step_frames_device(None, 1, 16, None, None, None, None, None, None, None, None, None) == -1
    from dsact.engine import DsactEngine
    for name in ("cnn_acting_capture", "step_frames_device", "act_sample_device_counted"):
        assert callable(getattr(DsactEngine, name)), name


# ---- the recording image engine ------------------------------------------------------------------------------------------------------
class GraphCnnEngine(FakeCnnEngine):
    """FakeCnnEngine with the graph route's entry points: each is recorded, the row moves are made"""

    def __init__(self):
        super().__init__()
        self.eval_begin = lambda n, e: self.calls.append(("eval_begin", n, e))
        self.eval_poll = lambda: 0
        self.eval_read = lambda e: (np.zeros(e), np.zeros(e, np.int32))
        self.note_torch_writes = lambda p: None

    def cnn_acting_capture(self):
        self.calls.append(("cnn_acting_capture",))

    def act_counter_set(self, step):
        self.calls.append(("act_counter_set", int(step)))

    def act_counter_add(self, k):
        self.calls.append(("act_counter_add", int(k)))

    def act_sample_device_counted(self, obs, offset, action, clipped, logp):
        FakeCnnEngine.act_sample_device(self, obs, None, offset, action, clipped, logp)
        self.calls[-1] = ("act_sample_device_counted", obs.shape[0], int(offset), obs.dtype)

    def step_frames_device(self, obs2, rew, term, trunc, obs2_slot, rew_slot, term_slot, trunc_slot, ended):
        assert obs2.is_contiguous() and obs2.dim() == 4 and obs2.dtype == obs2_slot.dtype
        obs2_slot.copy_(obs2); rew_slot.copy_(rew); term_slot.copy_(term); trunc_slot.copy_(trunc)
        ended.copy_(term | trunc)
        self.calls.append(("step_frames_device", obs2.shape[0], obs2.dtype, int(obs2[0].numel()) * obs2.element_size()))

    def step_rows_device(self, *a):
        raise AssertionError("step_rows_device on image rows")

    def act_mode_device(self, obs, action):
        self.calls.append(("act_mode_device", obs.shape[0], obs.dtype, obs.data_ptr()))
        action.zero_()

    def eval_commit(self, rew, term, trunc, ended):
        ended.copy_(term | trunc)
        self.calls.append(("eval_commit",))


def _names(eng):
    return [c[0] for c in eng.calls]


def _sampler(env, eng, **over):
    from plugin import create_sampler
    return create_sampler(sampler_name="hip_tensor_env_sampler", env=env, networks=_networks(eng) if eng is not None else None, seed=3,
                          **over)


def _evaluator(env, eng, **over):
    from plugin import create_evaluator
    return create_evaluator(evaluator_name="hip_tensor_env_evaluator", eval_env=env, networks=_networks(eng) if eng is not None else None,
                            **over)


# ---- 2. the pair: accepted on an image engine, refused elsewhere -------------------------------------------------------------------
@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_both_classes_construct_on_an_image_engine(frames):
    from synth_tensor_blob_inplace import SynthTensorBlobInplace

    eng = GraphCnnEngine()
    smp = _sampler(SynthTensorBlobInplace(4, seed=3, frames=frames), eng, sample_batch_size=8, hip_graph_sample=True, hip_cnn_act=True)
    ev = _evaluator(SynthTensorBlobInplace(2, seed=3, frames=frames), eng, num_eval_episode=2, hip_graph_eval=True, hip_cnn_act=True)
    assert smp.graph_sample and smp.cnn_act and ev.graph_eval and ev.cnn_act
    assert eng.calls == []                                               # construction calls nothing
    # the capture_safe rule is unchanged: the parent fixture is refused by name
    from synth_tensor_blob import SynthTensorBlob
    with pytest.raises(NotImplementedError, match="SynthTensorBlob does not promise it"):
        _sampler(SynthTensorBlob(4, seed=3, frames=frames), eng, sample_batch_size=8, hip_graph_sample=True, hip_cnn_act=True)
    with pytest.raises(NotImplementedError, match="SynthTensorBlob does not promise it"):
        _evaluator(SynthTensorBlob(2, seed=3, frames=frames), eng, num_eval_episode=2, hip_graph_eval=True, hip_cnn_act=True)


class SafeNoEnv:
    """carries the attributes of the protocol and capture_safe; any reset / step fails the test"""
    num_envs, capture_safe = 4, True

    def __init__(self, act_dim=A):
        self.action_low, self.action_high = torch.full((act_dim,), -1.0), torch.full((act_dim,), 1.0)

    def reset(self, mask=None):
        raise AssertionError("env.reset before the refusal")

    def step(self, action):
        raise AssertionError("env.step before the refusal")


class NoMethods(FakeEngine):
    """an MLP engine whose every method call fails the test: attribute reads are allowed"""

    def __getattribute__(self, k):
        v = super().__getattribute__(k)
        if callable(v) and not k.startswith("__"):
            raise AssertionError("engine method %s read before the refusal" % k)
        return v


def test_the_pair_on_an_mlp_engine_is_refused_before_any_call():
    for make, kwarg, more in ((_sampler, "hip_graph_sample", dict(sample_batch_size=8)), (_evaluator, "hip_graph_eval", {})):
        eng = NoMethods(act_dim=A)
        with pytest.raises(NotImplementedError, match=r"hip_cnn_act.*drop it") as ex:
            make(SafeNoEnv(), eng, hip_cnn_act=True, **dict(more, **{kwarg: True}))
        assert kwarg in str(ex.value) and "MLP" in str(ex.value)
        # a CNN engine without the acting path is refused as well (there the kwarg pair has nothing to capture)
        off = FakeCnnEngine()
        off.cnn_act = False
        with pytest.raises(NotImplementedError, match="hip_cnn_act"):
            make(SafeNoEnv(), off, hip_cnn_act=True, **dict(more, **{kwarg: True}))
        assert off.calls == []


def test_a_policy_attached_later_is_refused_at_the_first_call_before_anything_runs():
    smp = _sampler(SafeNoEnv(), None, sample_batch_size=8, hip_graph_sample=True, hip_cnn_act=True)   # nothing to check yet
    ev = _evaluator(SafeNoEnv(), None, num_eval_episode=2, hip_graph_eval=True, hip_cnn_act=True)
    smp.networks, ev.networks = _networks(NoMethods(act_dim=A)), _networks(NoMethods(act_dim=A))
    with pytest.raises(NotImplementedError, match=r"hip_graph_sample=True with hip_cnn_act=True.*drop it"):
        smp.sample()
    with pytest.raises(NotImplementedError, match=r"hip_graph_eval=True with hip_cnn_act=True.*drop it"):
        ev.run_evaluation(0)
    # ... and an image engine attached later is accepted (the refusal on a CPU engine is the device's, which comes first in _setup)
    smp.networks = _networks(GraphCnnEngine())
    with pytest.raises(NotImplementedError, match="hip_graph_sample=True needs an engine on a GPU"):
        smp.sample()


# ---- 3. the calls ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def any_device(monkeypatch):
    """the eager warm-up of the graph route on the CPU device: the device check is stepped over"""
    import training.hip_tensor_evaluator as ev_mod
    import training.hip_tensor_sampler as smp_mod
    monkeypatch.setattr(smp_mod, "require_graph_device", lambda kwarg, dev: None)
    monkeypatch.setattr(ev_mod, "require_graph_device", lambda kwarg, dev: None)


@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_sampler_opts_in_once_per_engine_and_moves_image_rows_in_one_call(any_device, frames):
    from synth_tensor_blob import SynthTensorBlob
    from synth_tensor_blob_inplace import SynthTensorBlobInplace

    N, S, dt = 4, 8, getattr(torch, frames)
    row_bytes = int(np.prod(SHAPE)) * (1 if frames == "uint8" else 4)
    eng = GraphCnnEngine()
    smp = _sampler(SynthTensorBlobInplace(N, seed=3, frames=frames), eng, sample_batch_size=S, hip_graph_sample=True, hip_cnn_act=True)
    batch, _ = smp.sample()                                              # the eager warm-up: the body a capture records
    step = [("act_sample_device_counted", N, 0, dt), ("step_frames_device", N, dt, row_bytes)]
    assert eng.calls == [("set_act_rng", smp.act_seed), ("cnn_acting_capture",), ("act_counter_set", 0)] + step \
        + [("act_sample_device_counted", N, 1, dt), step[1], ("act_counter_add", 2)]
    assert smp.act_step == 2 and smp.graph_captures == 0
    # the rows are the plain sampler's on the plain fixture
    ref_eng = FakeCnnEngine()
    want, _ = _sampler(SynthTensorBlob(N, seed=3, frames=frames), ref_eng, sample_batch_size=S, hip_cnn_act=True).sample()
    assert "cnn_acting_capture" not in _names(ref_eng) and _names(ref_eng) == ["set_act_rng", "act_sample_device", "act_sample_device"]
    for x, y in zip(batch.device_columns, want.device_columns):
        assert x.dtype == y.dtype and torch.equal(x, y)
    # the same engine again: no second opt-in; another engine: one more
    eng.calls.clear()
    smp._graph_calls = 0                                                 # (the warm-up body once more: a capture needs a GPU)
    smp.sample()
    assert "cnn_acting_capture" not in _names(eng) and _names(eng).count("step_frames_device") == 2
    other = GraphCnnEngine()
    smp.networks = _networks(other)
    smp.sample()
    assert _names(other).count("cnn_acting_capture") == 1
    # without the graph kwarg nothing opts in, and an image engine is not asked to under hip_graph_sample alone either
    plain = GraphCnnEngine()
    _sampler(SynthTensorBlobInplace(N, seed=3, frames=frames), plain, sample_batch_size=S, hip_cnn_act=True).sample()
    assert _names(plain) == ["set_act_rng", "act_sample_device", "act_sample_device"]


class StridedBlob:
    """SynthTensorBlobInplace whose step hands back obs2 as a non-contiguous view of the same values"""
    capture_safe = True

    def __init__(self, inner):
        self.inner = inner
        self.num_envs, self.action_low, self.action_high = inner.num_envs, inner.action_low, inner.action_high

    def reset(self, mask=None):
        return self.inner.reset(mask)

    def step(self, action):
        obs2, r, te, tr = self.inner.step(action)
        view = obs2.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not view.is_contiguous() and torch.equal(view, obs2)
        return view, r, te, tr


def test_non_contiguous_image_rows_fall_back_to_the_copies(any_device):
    from synth_tensor_blob_inplace import SynthTensorBlobInplace

    N, S = 4, 8
    eng, ref = GraphCnnEngine(), GraphCnnEngine()
    got, _ = _sampler(StridedBlob(SynthTensorBlobInplace(N, seed=3, frames="uint8")), eng, sample_batch_size=S, hip_graph_sample=True,
                      hip_cnn_act=True).sample()
    want, _ = _sampler(SynthTensorBlobInplace(N, seed=3, frames="uint8"), ref, sample_batch_size=S, hip_graph_sample=True,
                       hip_cnn_act=True).sample()
    assert "step_frames_device" not in _names(eng) and _names(eng).count("act_sample_device_counted") == 2
    assert _names(ref).count("step_frames_device") == 2
    for x, y in zip(got.device_columns, want.device_columns):
        assert torch.equal(x, y)


@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_evaluator_opts_in_once_and_reads_the_resets_frames_in_place(any_device, frames):
    from synth_tensor_blob_inplace import SynthTensorBlobInplace

    N, E, P = 2, 2, 20                                                   # an episode is 20 steps: one (eager, first) window
    eng = GraphCnnEngine()
    env = SynthTensorBlobInplace(N, seed=1, frames=frames)
    ev = _evaluator(env, eng, num_eval_episode=E, hip_graph_eval=True, hip_cnn_act=True, hip_eval_poll_steps=P)
    ev.run_evaluation(0)
    assert _names(eng).count("cnn_acting_capture") == 1 and eng.calls[0] == ("cnn_acting_capture",)
    modes = [c for c in eng.calls if c[0] == "act_mode_device"]
    assert len(modes) == P and all(c[1:3] == (N, getattr(torch, frames)) for c in modes)
    assert modes[0][3] == ev._obs.data_ptr()                             # a window starts from the evaluator's buffer
    if frames == "uint8":                                                # ... and goes on in the environment's own frames
        assert all(c[3] == env.codes.data_ptr() for c in modes[1:])
    else:
        assert all(c[3] != ev._obs.data_ptr() and c[3] % 16 == 0 for c in modes[1:])
    ev._graph_windows = 0                                                # (the warm-up window once more: a capture needs a GPU)
    ev.run_evaluation(1)
    assert _names(eng).count("cnn_acting_capture") == 1                  # once per engine
    # without the kwarg: no opt-in, every acting call on the evaluator's own buffer
    plain = GraphCnnEngine()
    ev2 = _evaluator(SynthTensorBlobInplace(N, seed=1, frames=frames), plain, num_eval_episode=E, hip_cnn_act=True, hip_eval_poll_steps=P)
    ev2.run_evaluation(0)
    assert "cnn_acting_capture" not in _names(plain)
    assert all(c[3] == ev2._obs.data_ptr() for c in plain.calls if c[0] == "act_mode_device")


# ---- 4. the in-place fixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_the_inplace_blob_equals_the_plain_one_bit_for_bit_and_keeps_its_storage(frames):
    from synth_tensor_blob import SynthTensorBlob
    from synth_tensor_blob_inplace import SynthTensorBlobInplace

    N, steps = 5, 64
    g = torch.Generator().manual_seed(11)
    actions = [2 * torch.rand(N, A, generator=g) - 1 for _ in range(steps)]
    plain, inpl = SynthTensorBlob(N, seed=2, frames=frames), SynthTensorBlobInplace(N, seed=2, frames=frames)
    assert inpl.capture_safe is True and getattr(plain, "capture_safe", False) is not True
    state = (inpl.draw, inpl.t, inpl.target, inpl.codes)
    ptrs = tuple(s.data_ptr() for s in state)

    def same(x, y):
        return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)

    def in_place():
        now = (inpl.draw, inpl.t, inpl.target, inpl.codes)
        return all(a is b for a, b in zip(now, state)) and tuple(s.data_ptr() for s in now) == ptrs

    assert same(plain.reset(), inpl.reset().clone()) and in_place()
    restarts = torch.zeros(N, dtype=torch.int64)
    for step, a in enumerate(actions):
        x, y = plain.step(a), inpl.step(a)
        for u, v in zip(x, y):                                           # frames, rewards and both flags, every row
            assert same(u, v), step
        assert x[0].dtype == getattr(torch, frames) and x[1].dtype == torch.float32 and x[2].dtype == x[3].dtype == torch.bool
        ended = x[2] | x[3]
        if step % 7 == 3:                                                # rows also restart alone, off the 20-step grid
            ended = ended | (torch.arange(N) == step % N)
        restarts += ended.to(torch.int64)
        assert same(plain.reset(ended), inpl.reset(ended.clone())), step
        for u, v in zip((plain.draw, plain.t, plain.target, plain.codes), state):
            assert same(u, v), step
        assert in_place(), step
    assert int(restarts.min()) >= 2                                      # every row restarted through reset(mask) on the way
    sd = plain.state_dict()
    inpl.load_state_dict(sd)
    assert in_place() and same(inpl.codes, plain.codes)
