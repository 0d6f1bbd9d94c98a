"""The reference's image pipeline on tensor environments (training/hip_tensor_frame_pipe.py) -- the host
side, without a GPU.

  1. the torch route on the CPU == tests/golden/frame_pipe.npz, the reference's own CarRacing Env recorded by
     scripts/frame_pipe_golden.py: gray under the parity rule (|ours - golden| <= 2**-24 everywhere, bit equality on all but
     1e-4 of the elements), stack order, repeat sums, flags and the ended index exactly;
  2. the semantics at the corners == a plain-Python per-row restatement (`_restate` below), BITWISE;
  3. every refusal, made before any environment call;
  4. the run state: a mid-episode save resumes bit for bit, other parameters or shapes are refused;
  5. composition with wrap_tensor_env, and bind_engine reaching the inner wrapper;
  6. `hip_frame_pipe` on HipTensorEnvSampler / HipTensorEnvEvaluator: routing and refusals;
  7. the two entry points are declared, exported and bound.
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

GOLDEN = os.path.join(HERE, "golden", "frame_pipe.npz")


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint8 if a.dtype == np.bool_ else np.uint32 if a.dtype == np.float32 else a.dtype)


def _pipe(*args, **kw):
    from training.hip_tensor_frame_pipe import frame_pipe_tensor_env

    return frame_pipe_tensor_env(*args, **kw)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def test_torch_route_equals_the_reference_recording():
    from synth_tensor_rgb import SynthTensorRgb

    g = np.load(GOLDEN)
    n, T, K, H, W = g["stack"].shape
    R = 4
    assert (n, T, K, H, W) == (7, 24, 4, 8, 12)
    ended = g["ended_at"]
    # the recording holds every phase of a repeat
    assert (ended == 0).any() and ((ended > 0) & (ended < R - 1)).any() and (ended == R - 1).any() and (ended == -1).any()
    assert np.array_equal(ended >= 0, g["done"])
    env = _pipe(SynthTensorRgb(n, height=H, width=W, layout="hwc", frames="uint8"), gray="hwc", frame_stack=K, action_repeat=R)
    assert not env.fused and not hasattr(env, "obs_shape") and env.frame_stack == K and env.action_repeat == R
    obs = env.reset()
    assert env.obs_shape == (K, H, W)                               # (the fixture names no row shape: known from the first rows)
    differ = total = restarted = 0

    def gray_close(ours, gold):
        nonlocal differ, total
        assert ours.dtype == torch.float32 and tuple(ours.shape) == gold.shape
        assert float(np.abs(ours.numpy().astype(np.float64) - gold.astype(np.float64)).max()) <= 2.0 ** -24      # condition one
        differ += int((_bits(ours) != _bits(gold)).sum())
        total += gold.size

    for s in range(T):
        gray_close(obs, g["start"][:, s])
        if s == 0 or g["done"][:, s - 1].any():
            rows = np.arange(n) if s == 0 else np.nonzero(g["done"][:, s - 1])[0]
            for r in rows:                                         # a restarted row shows K copies of its reset frame
                assert all(np.array_equal(_bits(obs[r, k]), _bits(obs[r, 0])) for k in range(K)), (s, r)
                assert all(np.array_equal(g["start"][r, s, k], g["start"][r, s, 0]) for k in range(K)), (s, r)
                restarted += 1
        obs2, rew, term, trunc = env.step(torch.from_numpy(g["action"][:, s]))
        gray_close(obs2, g["stack"][:, s])
        assert rew.dtype == torch.float32 and np.array_equal(_bits(rew), _bits(g["reward"][:, s])), s
        assert np.array_equal((term | trunc).numpy(), g["done"][:, s]) and not trunc.any(), s
        assert np.array_equal(env.ended_at.numpy(), ended[:, s]), s
        # stack order: the older slots are the start stack's newer ones, bit for bit (a move, no arithmetic)
        assert np.array_equal(_bits(obs2[:, :K - 1]), _bits(obs[:, 1:])), s
        obs = env.reset(term | trunc)
    assert restarted > n
    assert differ <= 1e-4 * total, (differ, total)                                                                # condition two


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def _gray_rule(frame, layout):
    """the sequential float64 rule in NumPy scalars' arithmetic, one rounded operation each"""
    x = frame.astype(np.float64)
    r, g, b = (x[0], x[1], x[2]) if layout == "chw" else (x[..., 0], x[..., 1], x[..., 2])
    return ((((r * 0.299 + g * 0.587) + b * 0.114) / 128.0) - 1.0).astype(np.float32)


def _restate(r, shape, dtype, gray, K, R, actions, limit):
    """environment r alone, in plain Python: per outer step (start stack, returned stack, reward, terminated, truncated, ended_at);
    a row that ended restarts before the next step"""
    from synth_tensor_rgb import rows_value

    def slot(k, t):
        frame = rows_value(r, k, t, shape, dtype)
        return (_gray_rule(frame, gray) if gray else frame).reshape(-1)

    k = t = 0
    stack = [slot(k, t)] * K
    out = []
    for act in actions:
        start = np.concatenate(stack)
        alive, acc, term, trunc, ended, last = True, None, False, False, -1, None
        for j in range(R):
            t += 1                                                  # the inner environment is stepped, alive or not
            rew = np.float32((37 * r + 101 * t + 11) % 64) * np.float32(1.0 / 16.0)
            sq = np.float32(0.0)
            for d in range(1, len(act)):
                sq = sq + act[d] * act[d]
            rew = np.float32(rew + sq)
            te, tr = (5 * r + 3 * k + t) % 13 == 0, t >= limit
            if alive:
                last = slot(k, t)
                acc = rew if j == 0 else np.float32(acc + rew)
                if te or tr:
                    alive, term, trunc, ended = False, te, tr, j
        stack = stack[1:] + [last]
        out.append((start, np.concatenate(stack), acc, term, trunc, ended))
        if ended >= 0:
            k, t = k + 1, 0
            stack = [slot(k, t)] * K
    return out


FORMS = [("chw-u8", (3, 5, 7), "uint8", "chw"), ("hwc-u8", (5, 7, 3), "uint8", "hwc"), ("chw-f32", (3, 5, 7), "float32", "chw"),
         ("hwc-f32", (5, 7, 3), "float32", "hwc"), ("codes", (1, 5, 7), "uint8", None), ("frames-f32", (2, 5, 7), "float32", None),
         ("vector", (6,), "float32", None)]


def _actions(N, steps):
    return [torch.from_numpy((((7 * np.arange(N)[:, None] + 3 * s + 5 * np.arange(3)[None, :]) % 9 - 4) * 0.1).astype(np.float32))
            for s in range(steps)]


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_semantics_equal_the_per_row_restatement(K, R, N):
    from synth_tensor_rgb import SynthTensorRows

    steps, limit = 14, 7
    acts = _actions(N, steps)
    for name, shape, dtype, gray in FORMS:
        inner = SynthTensorRows(N, shape, dtype, limit=limit)
        env = _pipe(inner, gray=gray, frame_stack=K, action_repeat=R)
        want = [_restate(r, shape, dtype, gray, K, R, [a[r].numpy() for a in acts], limit) for r in range(N)]
        obs = env.reset()
        shape_out = (K,) + (shape[1:] if gray == "chw" else shape[:2]) if gray else (K * shape[0],) + shape[1:]
        assert env.obs_shape == shape_out and tuple(obs.shape) == (N,) + shape_out, name
        assert obs.dtype == (torch.float32 if gray or dtype == "float32" else torch.uint8), name
        seen = set()
        for s in range(steps):
            kept = obs.clone()
            calls = inner.calls
            obs2, rew, term, trunc = env.step(acts[s])
            assert inner.calls == calls + R, name                   # exactly R inner steps, no inner reset
            assert obs.data_ptr() != obs2.data_ptr() and np.array_equal(_bits(obs), _bits(kept)), name      # reset's return survives the step
            for r in range(N):
                start, stack, acc, te, tr, ended = want[r][s]
                assert np.array_equal(_bits(kept[r].reshape(-1)), _bits(start)), (name, s, r)
                assert np.array_equal(_bits(obs2[r].reshape(-1)), _bits(stack)), (name, s, r)
                assert np.array_equal(_bits(rew[r:r + 1]), _bits(np.array([acc], np.float32))), (name, s, r)
                assert (bool(term[r]), bool(trunc[r]), int(env.ended_at[r])) == (te, tr, ended), (name, s, r)
                seen.add((ended, te, tr))
            next_kept = obs2.clone()
            ended = term | trunc
            before = env.stack.clone()
            obs = env.reset(ended)
            assert np.array_equal(_bits(obs2), _bits(next_kept)), name                                        # obs2 survives the reset(mask)
            keep = ~ended
            assert np.array_equal(_bits(obs[keep]), _bits(before[keep])) and np.array_equal(_bits(env.stack), _bits(obs)), name
        if N == 5:                                                   # rows ended at every inner index, by either flag, and not at all
            assert {e for e, _, _ in seen} == set(range(-1, R)), (name, seen)
            assert any(te for _, te, _ in seen) and any(tr for _, _, tr in seen), (name, seen)


def test_a_row_stepped_after_its_end_contributes_nothing():
    from synth_tensor_rgb import SynthTensorRows, ends_at

    # row 0's first episode terminates at t = 13, row 1's at t = 8: with R = 10 row 1 ends at inner index 7 and is stepped twice more
    assert (ends_at(0, 0), ends_at(1, 0)) == (13, 8)
    inner = SynthTensorRows(2, (6,), "float32")
    env = _pipe(inner, frame_stack=2, action_repeat=10)
    env.reset()
    act = torch.zeros(2, 3)
    obs2, rew, term, trunc = env.step(act)
    alone = SynthTensorRows(2, (6,), "float32")
    alone.reset()
    total, frame = None, None
    for j in range(8):
        frame, r, _, _ = alone.step(act)
        total = r.clone() if total is None else total + r
    assert env.ended_at.tolist() == [-1, 7] and term.tolist() == [False, True]
    assert np.array_equal(_bits(rew[1:]), _bits(total[1:])) and np.array_equal(_bits(obs2[1, 6:]), _bits(frame[1]))
    assert int(inner.t[1]) == 10                                     # ... while the inner environment was stepped all ten times


def test_all_none_is_the_environment_itself_and_attributes_forward():
    from synth_tensor_rgb import SynthTensorRgb

    inner = SynthTensorRgb(3)
    assert _pipe(inner) is inner and _pipe(inner, None, None, None) is inner
    env = _pipe(inner, gray="chw")                                   # frame_stack=None with gray: K = 1
    assert env.frame_stack == 1 and env.action_repeat == 1 and env.num_envs == 3 and env.capture_safe is True
    assert env.action_low is inner.action_low and env.action_high is inner.action_high and env.env is inner
    assert tuple(env.reset().shape) == (3, 1, 8, 12) and env.obs_shape == (1, 8, 12) and env.obs_dim == 96
    with pytest.raises(AttributeError):
        env.no_such_attribute
    inner.obs_shape = (3, 8, 12)                                     # a named row shape gives obs_shape before the first reset()
    assert _pipe(inner, gray="chw", frame_stack=4).obs_shape == (4, 8, 12) and _pipe(inner, frame_stack=4).obs_shape == (12, 8, 12)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(gray="rgb"), dict(gray=True), dict(gray=1), dict(gray="CHW"),
    dict(frame_stack=0), dict(frame_stack=-1), dict(frame_stack=2.0), dict(frame_stack=True), dict(frame_stack="4"), dict(frame_stack=65),
    dict(action_repeat=0), dict(action_repeat=-2), dict(action_repeat=1.5), dict(action_repeat=False), dict(action_repeat="4"),
    dict(gray="chw", frame_stack=0), dict(frame_stack=4, action_repeat=0),
])
def test_refusals_come_before_any_environment_call(kw):
    from synth_tensor_rgb import SynthTensorRows

    inner = SynthTensorRows(2, (3, 5, 7), "uint8")
    with pytest.raises(ValueError):
        _pipe(inner, **kw)
    assert inner.calls == 0
    assert _pipe(inner, frame_stack=64).frame_stack == 64


def test_first_rows_that_gray_cannot_take_are_refused():
    from synth_tensor_rgb import SynthTensorRows

    for shape, layout in (((5, 7, 3), "chw"), ((3, 5, 7), "hwc"), ((1, 5, 7), "chw"), ((6,), "hwc"), ((4, 5, 7), "chw")):
        with pytest.raises(ValueError, match="3-channel"):
            _pipe(SynthTensorRows(2, shape, "uint8"), gray=layout).reset()
    with pytest.raises(TypeError, match="uint8"):
        _pipe(SynthTensorRows(2, (3, 5, 7), "float64"), gray="chw").reset()


class _RecordingEngine:
    """an engine stub that keeps which calls the fused route makes (it computes nothing)"""
    stream_ptr = 0

    def __init__(self):
        self.calls = []

    def frame_pipe_reset(self, n, frame_stack, gray, raw, mask, stack, obs_out):
        self.calls.append(("reset", n, frame_stack, gray, mask is not None))

    def frame_pipe_step(self, n, j, action_repeat, frame_stack, gray, raw, *rest):
        self.calls.append(("step", n, j, action_repeat, frame_stack, gray))


def test_the_fused_route_never_changes_quietly():
    from synth_tensor_rgb import SynthTensorRows

    class Odd(SynthTensorRows):
        def step(self, action):
            raw, rew, term, trunc = super().step(action)
            return raw, rew.to(torch.float64), term, trunc

    env = _pipe(Odd(2, (3, 5, 7), "uint8"), gray="chw", action_repeat=2)
    env.reset()
    eng = _RecordingEngine()
    env.bind_engine(eng)
    assert env.fused
    with pytest.raises(TypeError, match="rewards"):
        env.step(torch.zeros(2, 3))
    assert eng.calls == []
    env.use_fused = False                                            # the torch route takes it (and casts)
    assert not env.fused and env.step(torch.zeros(2, 3))[1].dtype == torch.float32
    plain = _pipe(SynthTensorRows(2, (6,), "float64"), frame_stack=2)   # without gray any dtype passes through on the torch route
    assert plain.reset().dtype == torch.float64
    plain.bind_engine(eng)
    with pytest.raises(TypeError, match="uint8 or float32"):
        plain.step(torch.zeros(2, 3))
    good = _pipe(SynthTensorRows(2, (3, 5, 7), "uint8"), gray="chw", frame_stack=2, action_repeat=3)
    good.reset()
    good.bind_engine(eng)
    good.step(torch.zeros(2, 3))
    good.reset(torch.tensor([True, False]))
    assert eng.calls == [("step", 2, j, 3, 2, "chw") for j in range(3)] + [("reset", 2, 2, "chw", True)]


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_and_parameter_check():
    from synth_tensor_rgb import SynthTensorRgb

    N, kw = 5, dict(gray="chw", frame_stack=4, action_repeat=2)

    def drive(env, first, steps):
        out = []
        for act in _actions(N, first + steps)[first:]:
            res = env.step(act)
            out.append([t.clone() for t in res] + [env.ended_at.clone()])
            out.append([env.reset(res[2] | res[3]).clone()])
        return out

    a = _pipe(SynthTensorRgb(N), **kw)
    a.reset()
    drive(a, 0, 2)                                                   # two pushes into a stack of four: half filled
    sd = a.state_dict()
    assert sorted(sd) == ["format", "inner", "params", "stack"] and sd["format"] == "dsact-tensor-frame-pipe-state/1"
    assert sd["stack"].device.type == "cpu" and tuple(sd["stack"].shape) == (N, 4, 8, 12)
    half = sd["stack"][0]
    assert torch.equal(half[0], half[1]) and not torch.equal(half[1], half[2]) and not torch.equal(half[2], half[3])
    b = _pipe(SynthTensorRgb(N), **kw)
    b.reset()
    where = b.stack.data_ptr()
    b.load_state_dict(sd)
    assert b.stack.data_ptr() == where and torch.equal(b.stack, a.stack)
    for x, y in zip(drive(a, 2, 10), drive(b, 2, 10)):
        for u, v in zip(x, y):
            assert np.array_equal(_bits(u), _bits(v))
    for over in (dict(frame_stack=2), dict(action_repeat=3), dict(gray="hwc")):
        c = _pipe(SynthTensorRgb(N, layout=dict(kw, **over)["gray"]), **dict(kw, **over))
        c.reset()
        with pytest.raises(ValueError, match="pipeline was"):
            c.load_state_dict(sd)
    wide = _pipe(SynthTensorRgb(N, width=16), **kw)                  # the same parameters, another frame
    wide.reset()
    with pytest.raises(ValueError, match="saved stack"):
        wide.load_state_dict(sd)
    with pytest.raises(ValueError, match="not a"):
        b.load_state_dict({"format": "other"})

    class Bare:                                                      # no state_dict() of its own
        num_envs = 2

        def reset(self, mask=None):
            return torch.zeros(2, 6)

    bare = _pipe(Bare(), frame_stack=2)
    bare.reset()
    with pytest.raises(NotImplementedError, match="state_dict"):
        bare.state_dict()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_composition_inside_wrap_tensor_env():
    from synth_tensor_rgb import SynthTensorRows
    from training.hip_tensor_env_wrappers import wrap_tensor_env

    N, K, R, M, steps = 5, 2, 3, 3, 12
    shape, dtype, gray = (3, 5, 7), "uint8", "chw"
    inner = SynthTensorRows(N, shape, dtype)
    pipe = _pipe(inner, gray=gray, frame_stack=K, action_repeat=R)
    env = wrap_tensor_env(pipe, max_episode_steps=M, reward_shift=0.25, obs_scale=0.5)
    assert env.env is pipe and env.frame_stack == K and env.action_repeat == R
    acts = _actions(N, steps)
    obs = env.reset()
    # the restatement: every row alone; the limit counts OUTER steps, so a row restarts after M held actions at the latest
    elapsed, rows = [0] * N, []
    for r in range(N):
        rows.append({"k": 0, "t": 0})
    limited = 0
    from synth_tensor_rgb import rows_value
    stacks = [[_gray_rule(rows_value(r, 0, 0, shape, dtype), gray).reshape(-1)] * K for r in range(N)]
    for s in range(steps):
        obs2, rew, term, trunc = env.step(acts[s])
        for r in range(N):
            st = rows[r]
            alive, acc, te_out, last = True, None, False, None
            for j in range(R):
                st["t"] += 1
                rj = np.float32(np.float32((37 * r + 101 * st["t"] + 11) % 64) * np.float32(1.0 / 16.0)
                                + (np.float32(0.0) + acts[s][r, 1].numpy() ** 2 + acts[s][r, 2].numpy() ** 2))
                if alive:
                    last = _gray_rule(rows_value(r, st["k"], st["t"], shape, dtype), gray).reshape(-1)
                    acc = rj if j == 0 else np.float32(acc + rj)
                    if (5 * r + 3 * st["k"] + st["t"]) % 13 == 0:
                        alive, te_out = False, True
            stacks[r] = stacks[r][1:] + [last]
            elapsed[r] += 1
            hit = elapsed[r] >= M
            assert bool(term[r]) == te_out and bool(trunc[r]) == (hit and not te_out), (s, r)
            limited += hit and not te_out
            assert np.array_equal(_bits(rew[r:r + 1]), _bits(np.array([(acc + np.float32(0.25)) * np.float32(1.0)], np.float32))), (s, r)
            assert np.array_equal(_bits(obs2[r].reshape(-1)), _bits((np.concatenate(stacks[r]) + np.float32(0.0)) * np.float32(0.5))), (s, r)
            if te_out or hit:
                st["k"], st["t"], elapsed[r] = st["k"] + 1, 0, 0
                stacks[r] = [_gray_rule(rows_value(r, st["k"], 0, shape, dtype), gray).reshape(-1)] * K
        obs = env.reset(term | trunc)
        assert env.elapsed.tolist() == elapsed
        for r in range(N):
            assert np.array_equal(_bits(obs[r].reshape(-1)), _bits((np.concatenate(stacks[r]) + np.float32(0.0)) * np.float32(0.5))), (s, r)
    assert limited > 0
    # uint8 stacks are still refused by obs_scale
    with pytest.raises(NotImplementedError, match="uint8"):
        wrap_tensor_env(_pipe(SynthTensorRows(2, (1, 5, 7), "uint8"), frame_stack=2), obs_scale=2.0).reset()
    # bind_engine on the outer wrapper reaches the inner one
    eng = _RecordingEngine()
    assert not pipe.fused
    env.bind_engine(eng)
    assert pipe._engine is eng and pipe.fused and env.fused
    env.bind_engine(None)
    assert not pipe.fused and not env.fused


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
class PipeEngine(FakeEngine):
    """FakeEngine whose two frame-pipe calls are restated by a torch-route twin of the wrapper stepping the SAME inner rows"""

    def act_mode_device(self, obs, action):
        action.zero_()

    def frame_pipe_reset(self, n, frame_stack, gray, raw, mask, stack, obs_out):
        self.calls.append(("frame_pipe_reset", n, frame_stack, gray, mask is not None))
        new = raw.reshape(n, 1, -1)
        slots = stack.view(n, frame_stack, -1)
        slots.copy_(new.expand_as(slots) if mask is None else torch.where(mask[:, None, None], new, slots))
        obs_out.copy_(stack)

    def frame_pipe_step(self, n, j, action_repeat, frame_stack, gray, raw, rew, terminated, truncated, stack, acc, ended_at, flags,
                        obs2_out, rew_out, terminated_out, truncated_out):
        self.calls.append(("frame_pipe_step", n, j, action_repeat, frame_stack, gray))
        slots = stack.view(n, frame_stack, -1)
        alive = torch.ones(n, dtype=torch.bool) if j == 0 else ended_at < 0
        if j == 0:
            slots[:, :-1].copy_(slots[:, 1:].clone())
            acc.copy_(rew)
            terminated_out.zero_()
            truncated_out.zero_()
            ended_at.fill_(-1)
        else:
            acc.copy_(torch.where(alive, acc + rew, acc))
        slots[:, -1].copy_(torch.where(alive[:, None], raw.reshape(n, -1), slots[:, -1]))
        ends = alive & (terminated | truncated)
        terminated_out.copy_(torch.where(ends, terminated, terminated_out))
        truncated_out.copy_(torch.where(ends, truncated, truncated_out))
        ended_at.masked_fill_(ends, j)
        rew_out.copy_(acc)
        obs2_out.copy_(stack)


def _piped_sampler(eng, N=4, S=8, **over):
    from plugin import create_sampler
    from synth_tensor_rgb import SynthTensorRows

    inner = SynthTensorRows(N, (17,), "float32")
    kw = dict(sampler_name="hip_tensor_env_sampler", env=inner, sample_batch_size=S, networks=_networks(eng), seed=3)
    return create_sampler(**dict(kw, **over)), inner


def test_hip_frame_pipe_on_the_sampler():
    from training.hip_tensor_env_wrappers import WrappedTensorEnv
    from training.hip_tensor_frame_pipe import FramePipeTensorEnv

    eng = FakeEngine(obs_dim=17, act_dim=3)
    smp, inner = _piped_sampler(eng, frame_stack=2, action_repeat=3)
    assert smp.env is inner                                          # the default is off: the environment as it came
    smp, inner = _piped_sampler(eng, hip_frame_pipe=False, frame_stack=2)
    assert smp.env is inner
    eng = PipeEngine(obs_dim=34, act_dim=3)
    smp, inner = _piped_sampler(eng, hip_frame_pipe=True, frame_stack=2, action_repeat=3)
    env = smp.env
    assert isinstance(env, FramePipeTensorEnv) and env.env is inner and (env.frame_stack, env.action_repeat, env._gray) == (2, 3, None)
    assert not env.fused
    batch, _ = smp.sample()                                          # _setup binds the engine behind the first reset()
    assert env.fused and env._engine is eng
    pipes = [c for c in eng.calls if c[0].startswith("frame_pipe")]
    assert pipes == ([("frame_pipe_step", 4, j, 3, 2, None) for j in range(3)] + [("frame_pipe_reset", 4, 2, None, True)]) * 2
    ref, _ = _piped_sampler(FakeEngine(obs_dim=34, act_dim=3), hip_frame_pipe=True, frame_stack=2, action_repeat=3)
    ref.env.use_fused = False                                        # (FakeEngine has no frame-pipe calls: any would raise)
    want, _ = ref.sample()
    for u, v in zip(batch.device_columns, want.device_columns):
        assert np.array_equal(_bits(u), _bits(v))
    assert tuple(batch.device_columns[0].shape) == (8, 34)
    # before hip_env_wrap: the pipeline sits inside the wrappers
    smp, inner = _piped_sampler(PipeEngine(obs_dim=34, act_dim=3), hip_frame_pipe=True, frame_stack=2, hip_env_wrap=True, max_episode_steps=5)
    assert isinstance(smp.env, WrappedTensorEnv) and isinstance(smp.env.env, FramePipeTensorEnv) and smp.env.env.env is inner
    smp, _ = _piped_sampler(eng, hip_frame_pipe=True, frame_gray=None, action_repeat=2)
    assert (smp.env.frame_stack, smp.env.action_repeat) == (1, 2)
    for bad in ("yes", 1, None, 0):
        with pytest.raises(ValueError, match="hip_frame_pipe must be"):
            _piped_sampler(eng, hip_frame_pipe=bad, frame_stack=2)
    with pytest.raises(ValueError, match="does nothing"):
        _piped_sampler(eng, hip_frame_pipe=True)
    with pytest.raises(ValueError, match="frame_stack"):
        _piped_sampler(eng, hip_frame_pipe=True, frame_stack=0)
    with pytest.raises(ValueError, match="gray"):
        _piped_sampler(eng, hip_frame_pipe=True, frame_gray="rgb")


def test_hip_frame_pipe_on_the_evaluator():
    from plugin import create_evaluator
    from synth_tensor_rgb import SynthTensorRows, ends_at
    from training.hip_tensor_frame_pipe import FramePipeTensorEnv

    N, E, R = 4, 8, 3

    class EvalEngine(PipeEngine):
        """PipeEngine with the evaluation bookkeeping in Python"""

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
        inner = SynthTensorRows(N, (17,), "float32")
        kw = dict(evaluator_name="hip_tensor_env_evaluator", eval_env=inner, num_eval_episode=E, networks=_networks(eng))
        return create_evaluator(**dict(kw, **over)), inner

    ev, inner = make(EvalEngine(obs_dim=17, act_dim=3), frame_stack=2, action_repeat=R)
    assert ev.env is inner
    eng = EvalEngine(obs_dim=34, act_dim=3)
    ev, inner = make(eng, hip_frame_pipe=True, frame_stack=2, action_repeat=R)
    assert isinstance(ev.env, FramePipeTensorEnv) and ev.env.action_repeat == R      # the evaluator keeps the repeat
    ev.run_evaluation(0)
    assert ev.env.fused and any(c[0] == "frame_pipe_step" for c in eng.calls)
    # lengths count outer steps: an episode that terminates at inner step t lasts ceil(t / R) held actions
    assert ev.lengths.tolist() == [-(-ends_at(e % N, e // N) // R) for e in range(E)]
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="hip_frame_pipe must be"):
            make(eng, hip_frame_pipe=bad, frame_stack=2)
    with pytest.raises(ValueError, match="does nothing"):
        make(eng, hip_frame_pipe=True)


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    import ctypes as C

    from dsact import _ffi

    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    P = C.c_void_p
    want = {
        "dsact_frame_pipe_step": (r"int dsact_frame_pipe_step\(dsact_handle\* h, int32_t n, int64_t slot_elems, int32_t frame_stack, "
                                  r"int32_t action_repeat, int32_t j,\s+int32_t gray, int32_t elem_size, const void\* raw_dev, "
                                  r"const float\* rew_dev, const uint8_t\* terminated_dev,\s+const uint8_t\* truncated_dev, "
                                  r"void\* stack_dev, float\* acc_dev, int32_t\* ended_at_dev, uint8_t\* flags_dev,\s+void\* obs2_out, "
                                  r"float\* rew_out, uint8_t\* terminated_out, uint8_t\* truncated_out\);",
                                  [P, C.c_int32, C.c_int64] + [C.c_int32] * 5 + [P] * 12),
        "dsact_frame_pipe_reset": (r"int dsact_frame_pipe_reset\(dsact_handle\* h, int32_t n, int64_t slot_elems, int32_t frame_stack, "
                                   r"int32_t gray, int32_t elem_size,\s+const void\* raw_dev, const uint8_t\* mask_dev, void\* stack_dev, "
                                   r"void\* obs_out\);", [P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, P, P, P, P]),
    }
    bound = {n: (res, args) for n, res, args in _ffi.SYMBOLS}
    for name, (decl, args) in want.items():
        assert re.search(decl, hdr), name
        assert bound[name] == (C.c_int, args), name
    assert '"frame_pipe_calls"' in hdr
    lib = _ffi.load()
    for name in want:
        assert hasattr(lib, name), name
    # without a handle the entry points refuse like every other one
    assert lib.dsact_frame_pipe_step(None, 1, 1, 1, 1, 0, 0, 4, *([None] * 12)) == -1
    assert lib.dsact_frame_pipe_reset(None, 1, 1, 1, 0, 4, None, None, None, None) == -1
