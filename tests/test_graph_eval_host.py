"""The tensor evaluator's poll windows as one captured graph (training/hip_tensor_evaluator.py with hip_graph_eval=True, DESIGN.md
section 23) -- the host side, without a GPU.

  1. the constructor's refusals come before the environment is reset or stepped and before the engine is called; an engine off
     the GPU is refused at the first run_evaluation;
  2. tests/envs/synth_tensor_episodes_inplace.py equals tests/envs/synth_tensor_episodes.py bit for bit over 64 lockstep steps
     with restarts through reset(mask), and its state tensors keep their storage;
  3. without the kwarg the evaluator makes exactly the calls it always made, on its own staging buffers;
  4. the window body with the staging copies off the chain hands the environment's tensors through and computes the same
     evaluation;
  5. the header says what holds under capture.
"""
import os
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

from test_tensor_evaluator_host import FakeEngine, _networks   # noqa: E402

O, A = 17, 6


# ---- 1. refusals ---------------------------------------------------------------------------------------------------------------------
class RecordingEngine(FakeEngine):
    """FakeEngine whose every entry point is recorded, the ones the evaluator has no business calling included"""

    def note_torch_writes(self, params):
        self.calls.append(("note_torch_writes",))

    def debug_get(self, name):
        self.calls.append(("debug_get", name))
        return 0.0


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
    from plugin import create_evaluator
    kw = dict(dict(num_eval_episode=4), **over)
    return create_evaluator(evaluator_name="hip_tensor_env_evaluator", eval_env=env, networks=_networks(eng), **kw)


def test_refusals_come_before_any_environment_or_engine_call():
    for attrs in ({}, {"capture_safe": False}, {"capture_safe": 1}):      # absent, False, and truthy-but-not-True
        env, eng = RecordingEnv(**attrs), RecordingEngine()
        with pytest.raises(NotImplementedError, match="capture_safe"):
            _create(env, eng, hip_graph_eval=True)
        assert env.calls == [] and eng.calls == []
    env, eng = RecordingEnv(capture_safe=True), RecordingEngine()
    with pytest.raises(NotImplementedError, match="hip_cnn_act"):
        _create(env, eng, hip_graph_eval=True, hip_cnn_act=True)
    assert env.calls == [] and eng.calls == []
    for bad in (1, 0, "yes", None, 1.0):
        env, eng = RecordingEnv(capture_safe=True), RecordingEngine()
        with pytest.raises(ValueError, match="hip_graph_eval"):
            _create(env, eng, hip_graph_eval=bad)
        assert env.calls == [] and eng.calls == []
    # the parent of the in-place fixture rebinds its state: it does not carry the attribute and is refused by name
    from synth_tensor_episodes import SynthTensorEpisodes
    with pytest.raises(NotImplementedError, match="SynthTensorEpisodes does not promise it"):
        _create(SynthTensorEpisodes(5), RecordingEngine(), hip_graph_eval=True)


def test_an_engine_off_the_gpu_is_refused_at_the_first_run_evaluation():
    env, eng = RecordingEnv(capture_safe=True), RecordingEngine()
    ev = _create(env, eng, hip_graph_eval=True)                        # the constructor cannot know the engine's device yet
    assert ev.graph_eval and ev.graph_captures == 0 and ev.graph_replays == 0
    assert env.calls == [] and eng.calls == []
    with pytest.raises(NotImplementedError, match="hip_graph_eval=True needs an engine on a GPU"):
        ev.run_evaluation(0)
    assert env.calls == [] and eng.calls == []
    assert ev.graph_captures == 0 and ev.graph_replays == 0 and ev.steps == 0


# ---- 2. the in-place fixture ---------------------------------------------------------------------------------------------------------
def test_the_inplace_fixture_equals_the_plain_one_bit_for_bit_and_keeps_its_storage():
    from synth_tensor_episodes import SynthTensorEpisodes
    from synth_tensor_episodes_inplace import SynthTensorEpisodesInplace

    N, steps = 33, 64
    g = torch.Generator().manual_seed(11)
    actions = [0.8 * torch.rand(N, A, generator=g) - 0.4 for _ in range(steps)]
    plain, inpl = SynthTensorEpisodes(N), SynthTensorEpisodesInplace(N)
    assert inpl.capture_safe is True and getattr(plain, "capture_safe", False) is not True
    t, k = inpl.t, inpl.k
    ptrs = (t.data_ptr(), k.data_ptr())

    def same(x, y):
        return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)

    assert same(plain.reset(), inpl.reset())
    restarts = both = 0
    for step, a in enumerate(actions):
        x, y = plain.step(a), inpl.step(a)
        assert len(x) == len(y) == 4
        for u, v in zip(x, y):                                           # observations, rewards and both flags, every row
            assert same(u, v), step
        assert x[1].dtype == torch.float32 and x[2].dtype == x[3].dtype == torch.bool
        ended = x[2] | x[3]
        restarts += int(ended.sum())
        both += int((x[2] & x[3]).sum())
        assert same(plain.reset(ended), inpl.reset(ended.clone())), step
        assert torch.equal(plain.t, inpl.t) and torch.equal(plain.k, inpl.k)
        assert inpl.t is t and inpl.k is k and (inpl.t.data_ptr(), inpl.k.data_ptr()) == ptrs
    assert restarts > N and both >= 1 and int(inpl.k.min()) >= 1       # every row restarted through reset(mask) on the way
    inpl.reset()                                                         # ... and the full reset stays in place as well
    assert (inpl.t.data_ptr(), inpl.k.data_ptr()) == ptrs and not inpl.t.any() and not inpl.k.any()


# ---- 3. the kwarg off ------------------------------------------------------------------------------------------------------------------
class PointerEngine(RecordingEngine):
    """records which storage each acting call reads and each commit is handed"""

    def act_mode_device(self, obs, action):
        FakeEngine.act_mode_device(self, obs, action)
        self.calls[-1] = ("act_mode_device", obs.shape[0], obs.data_ptr(), action.data_ptr())

    def eval_commit(self, reward, terminated, truncated, ended):
        FakeEngine.eval_commit(self, reward, terminated, truncated, ended)
        self.calls[-1] = ("eval_commit", reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr(), ended.data_ptr())


@pytest.mark.parametrize("over", [{}, {"hip_graph_eval": False}])
def test_without_the_kwarg_the_call_sequence_is_todays(over):
    from synth_tensor_episodes import SynthTensorEpisodes
    from synth_tensor_episodes_inplace import SynthTensorEpisodesInplace

    N, E, P = 5, 7, 4
    for env in (SynthTensorEpisodes(N), SynthTensorEpisodesInplace(N)):  # (the attribute alone switches nothing on)
        eng = PointerEngine()
        ev = _create(env, eng, hip_eval_poll_steps=P, **dict(over, num_eval_episode=E))
        assert not getattr(ev, "graph_eval", False)                      # (getattr: the sequence below is also the parent commit's)
        ev.run_evaluation(0)
        steps = ev.steps
        assert steps == 16                                              # 13 lockstep steps are needed: four windows of 4
        # note_torch_writes, eval_begin, then per step the acting call on the evaluator's own observation buffer and the commit
        # on its own reward / flag buffers, a poll behind every P-th step, eval_read at the end -- and nothing else
        act = ("act_mode_device", N, ev._obs.data_ptr(), ev._act.data_ptr())
        commit = ("eval_commit", ev._rew.data_ptr(), ev._term.data_ptr(), ev._trunc.data_ptr(), ev._ended.data_ptr())
        want = [("note_torch_writes",), ("eval_begin", N, E)]
        for s in range(steps):
            want += [act, commit] + ([("eval_poll",)] if (s + 1) % P == 0 else [])
        want.append(("eval_read", E))
        assert eng.calls == want
        assert getattr(ev, "graph_captures", 0) == 0 and getattr(ev, "graph_replays", 0) == 0
    # hip_eval_max_steps off the window grid: the remainder is stepped, then polled once
    eng = PointerEngine()
    ev = _create(SynthTensorEpisodes(5), eng, hip_eval_poll_steps=4, hip_eval_max_steps=6, **dict(over, num_eval_episode=70))
    with pytest.raises(RuntimeError, match="hip_eval_max_steps = 6"):
        ev.run_evaluation(0)
    names = [c[0] for c in eng.calls]
    assert names == ["note_torch_writes", "eval_begin"] + ["act_mode_device", "eval_commit"] * 4 + ["eval_poll"] + \
        ["act_mode_device", "eval_commit"] * 2 + ["eval_poll"] and ev.steps == 6


# ---- 4. the window body of the kwarg-on route ---------------------------------------------------------------------------------------
def test_the_direct_window_hands_the_environments_tensors_through_and_computes_the_same():
    """_window is the one function both routes run; with graph_eval set it leaves the staging copies out. Driven here on the CPU
    with the fake engine (the route itself needs a GPU: test_graph_eval_gpu.py)."""
    from synth_tensor_episodes import SynthTensorEpisodes
    from synth_tensor_episodes_inplace import SynthTensorEpisodesInplace

    N, E, P = 5, 7, 4
    ref = _create(SynthTensorEpisodes(N), PointerEngine(), hip_eval_poll_steps=P, num_eval_episode=E)
    ref.run_evaluation(0)
    env, eng = SynthTensorEpisodesInplace(N), PointerEngine()
    ev = _create(env, eng, hip_eval_poll_steps=P, num_eval_episode=E)
    ev._setup(eng)
    ev.graph_eval = True                                                 # (the constructor's switch, past the GPU-only gate)
    eng.eval_begin(N, E)
    ev._obs.copy_(env.reset())
    del eng.calls[:]
    windows = 0
    while eng.eval_poll():
        ev._window(eng, P)
        windows += 1
        assert torch.equal(ev._obs, env._obs())                          # the fixed address holds the next window's observations
    assert windows * P == ref.steps
    returns, lengths = eng.eval_read(E)
    assert np.array_equal(returns.view(np.uint64), ref.returns.view(np.uint64)) and np.array_equal(lengths, ref.lengths)
    acts = [c for c in eng.calls if c[0] == "act_mode_device"]
    commits = [c for c in eng.calls if c[0] == "eval_commit"]
    assert len(acts) == len(commits) == windows * P
    own = {ev._rew.data_ptr(), ev._term.data_ptr(), ev._trunc.data_ptr()}
    for i, (a, c) in enumerate(zip(acts, commits)):
        assert (a[2] == ev._obs.data_ptr()) == (i % P == 0), i          # a window starts from the buffer, later steps read in place
        assert not own & set(c[1:4]) and c[4] == ev._ended.data_ptr(), i
    # anything but contiguous float32 / bool falls back to the three copies
    class Odd(SynthTensorEpisodesInplace):
        def step(self, action):
            obs2, r, te, tr = SynthTensorEpisodesInplace.step(self, action)
            return obs2, r.double(), te, tr
    env2, eng2 = Odd(N), PointerEngine()
    ev2 = _create(env2, eng2, hip_eval_poll_steps=P, num_eval_episode=E)
    ev2._setup(eng2)
    ev2.graph_eval = True
    eng2.eval_begin(N, E)
    ev2._obs.copy_(env2.reset())
    while eng2.eval_poll():
        ev2._window(eng2, P)
    assert all(c[1:4] == (ev2._rew.data_ptr(), ev2._term.data_ptr(), ev2._trunc.data_ptr()) for c in eng2.calls if c[0] == "eval_commit")
    assert np.array_equal(eng2.eval_read(E)[0].view(np.uint64), ref.returns.view(np.uint64))


# ---- 5. the header ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_capture_rules():
    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    doc = hdr[hdr.index("Device-resident evaluation"):hdr.index("int dsact_act_mode_device")]
    for word in ("UNDER STREAM CAPTURE", "LEGAL WHILE THE HANDLE'S STREAM IS CAPTURING", "make one call outside\n", "eval_state_gen",
                 "valid only for the generation it was captured under", "count HOST calls",
                 "dsact_eval_begin / dsact_eval_poll / dsact_eval_read   DSACT_E_STATE under capture"):
        assert word in doc, word
