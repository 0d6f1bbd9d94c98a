"""The reference's environment wrappers on tensor environments, on the GPU (k_env_wrap_step / k_env_wrap_reset,
dsact_env_wrap_step / dsact_env_wrap_reset, training/hip_tensor_env_wrappers.py). Everything is compared
BITWISE: the fused route is one launch that computes what the torch route's dozen ops compute, and
tests/test_env_wrap_host.py holds the torch route to the reference's recording.

  1. the kernels against the torch route on the same GPU tensors: every part alone and all together, scalar and per-element
     parameters, limits 1 and 5, NaN / inf / -0.0 / denormals, the 4-byte path forced by a view one float into its storage,
     in-place outputs, float32 frames on one wave and split over workgroups, masks of all zeros and all ones, the counter;
  2. the C-ABI's refusals are error returns that leave the handle usable;
  3. the sampler: fused == torch route == the integer plan, on the batch and on the ring rows; under hip_graph_sample;
  4. the evaluator: lengths == min(plan, M), returns sum the shifted reward, eager == hip_graph_eval == torch route; eval_save's
     default step bound;
  5. run_state() / load_run_state() of a wrapped sampler, cut in mid-episode;
  6. HipOffSerialTrainer with both wrapped routes captured ends bitwise equal to the torch route.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs
from test_hip_parity import make_pair

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

O, A, HID = 17, 6, (64, 64)
M = 5
RAMP = np.linspace(0.5, 1.5, O).astype(np.float32)
WRAP = dict(max_episode_steps=M, reward_shift=0.3, obs_shift=0.1, obs_scale=RAMP)


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint8 if a.dtype == np.bool_ else np.uint32 if a.dtype == np.float32 else a.dtype)


def _same(x, y, what):
    assert len(x) == len(y), what
    for k, (u, v) in enumerate(zip(x, y)):
        assert u.dtype == v.dtype and tuple(u.shape) == tuple(v.shape) and np.array_equal(_bits(u), _bits(v)), (what, k)


@pytest.fixture(scope="module")
def shared():
    """one engine for the cases that never write its weights"""
    alg, _ = make_pair(O, A, HID, 64, seed=4)
    return alg


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
class Script:
    """an 'environment' that hands out the tensors it was given: step -> (obs2, rew, term, trunc), reset -> raw"""

    def __init__(self, obs2, rew, term, trunc, raw):
        self.num_envs = int(rew.shape[0])
        self.out, self.raw = (obs2, rew, term, trunc), raw

    def reset(self, mask=None):
        return self.raw

    def step(self, action):
        return self.out


SPECIAL = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 1e-40, -1e-45, 3e-39, 3.4e38, -3.4e38]


def _rows(n, row, seed, offset=0):
    """float32 [n, *row] with special values among the normals, in a storage `offset` floats in"""
    g = torch.Generator().manual_seed(seed)
    numel = n * int(np.prod(row))
    flat = torch.randn(numel, generator=g) * 3.0
    where = torch.randperm(numel, generator=g)[:max(1, min(numel // 3, 200))]
    flat[where] = torch.tensor(SPECIAL, dtype=torch.float32)[torch.arange(where.numel()) % len(SPECIAL)]
    store = torch.zeros(numel + 8, device="cuda")
    store[offset:offset + numel].copy_(flat)
    return store[offset:offset + numel].view((n,) + tuple(row))


def _script(n, row, seed, offset=0):
    g = torch.Generator().manual_seed(seed + 1)
    rew = _rows(n, (1,), seed + 2).reshape(n).contiguous()
    term = (torch.rand(n, generator=g) < 0.3).cuda()
    trunc = (torch.rand(n, generator=g) < 0.3).cuda()
    return Script(_rows(n, row, seed + 3, offset), rew, term, trunc, _rows(n, row, seed + 4, offset))


def _params(row, per_element):
    if not per_element:
        return dict(obs_shift=0.1, obs_scale=-0.75)
    numel = int(np.prod(row))
    shift = np.linspace(-2.0, 2.0, numel).astype(np.float32).reshape(row)
    scale = np.linspace(-1.5, 1.5, numel).astype(np.float32).reshape(row)
    scale.reshape(-1)[::7] = 0.0                                     # inf * 0 and NaN * 0 among the products
    scale.reshape(-1)[3::11] = 3e-39                                 # products in the denormal range
    return dict(obs_shift=shift, obs_scale=scale)


def _configs(row):
    yield dict(max_episode_steps=1)
    yield dict(max_episode_steps=5)
    yield dict(reward_shift=0.3, reward_scale=0.7)
    yield dict(reward_scale=-3e-39)
    yield _params(row, False)
    yield _params(row, True)
    yield dict(_params(row, True), max_episode_steps=5, reward_shift=0.3, reward_scale=0.7)
    yield dict(_params(row, False), max_episode_steps=1, reward_shift=-1.0)


def _drive(eng, script, kw, fused, steps=7):
    """reset(), then `steps` x (step, reset(mask)) with masks of all zeros (four times: elapsed reaches 5), all ones and mixed:
    every returned tensor, cloned, plus elapsed; on the fused route under the engine's stream, with the launch counter checked"""
    from training.hip_tensor_env_wrappers import wrap_tensor_env

    env = wrap_tensor_env(script, **kw)
    n = script.num_envs
    out = []
    if fused:
        env.bind_engine(eng)
    else:
        env.use_fused = False
    assert env.fused == fused
    g = torch.Generator().manual_seed(9)
    masks = [torch.zeros(n, dtype=torch.bool)] * 4 + [torch.ones(n, dtype=torch.bool)] + [torch.rand(n, generator=g) < 0.5 for _ in range(steps)]
    masks = [m.cuda() for m in masks]
    act = torch.zeros(n, 1, device="cuda")
    torch.cuda.synchronize()
    obs_on, limit_on = "obs_scale" in kw, "max_episode_steps" in kw
    with torch.cuda.stream(eng.torch_stream):
        calls = eng.debug_get("env_wrap_calls")
        out.append([env.reset().clone()])
        calls += 1 if fused and (obs_on or limit_on) else 0
        assert eng.debug_get("env_wrap_calls") == calls
        for s in range(steps):
            res = env.step(act)
            calls += 1 if fused else 0
            assert eng.debug_get("env_wrap_calls") == calls
            out.append([t.clone() for t in res] + ([env.elapsed.clone()] if limit_on else []))
            out.append([env.reset(masks[s]).clone()] + ([env.elapsed.clone()] if limit_on else []))
            calls += 1 if fused and (obs_on or limit_on) else 0
            assert eng.debug_get("env_wrap_calls") == calls
        eng.sync()
    return out


@pytest.mark.parametrize("row", [1, 17, 376])
@pytest.mark.parametrize("n", [1, 3, 65, 1030])
def test_kernels_equal_the_torch_route(shared, n, row):
    eng = shared.engine
    for c, kw in enumerate(_configs((row,))):
        script = _script(n, (row,), seed=100 * c + n + row)
        want = _drive(eng, script, kw, False)
        got = _drive(eng, script, kw, True)
        for s, (x, y) in enumerate(zip(got, want)):
            _same(x, y, (c, s))
        if "max_episode_steps" in kw:                                # the counter reached the limit and, with M = 5, was below it
            seen = torch.stack([x[4] for x in want[1::2]])
            assert int(seen.max()) == kw["max_episode_steps"] and int(seen.min()) == 1
    assert eng.debug_get("act_dev_syncs") == 0.0 and eng.debug_get("handoff_failures") == 0.0


def test_the_four_byte_path_and_in_place_outputs(shared):
    eng = shared.engine
    n, row = 65, 376
    kw = dict(_params((row,), True), max_episode_steps=5, reward_shift=0.3, reward_scale=0.7)
    aligned, shifted = _script(n, (row,), seed=7), _script(n, (row,), seed=7, offset=1)
    assert aligned.out[0].data_ptr() % 16 == 0 and shifted.out[0].data_ptr() % 16 == 4 and shifted.out[0].is_contiguous()
    assert np.array_equal(_bits(aligned.out[0]), _bits(shifted.out[0]))
    want = _drive(eng, aligned, kw, False)
    for script in (aligned, shifted):                                # 16 bytes per lane, then 4
        for s, (x, y) in enumerate(zip(_drive(eng, script, kw, True), want)):
            _same(x, y, s)
    # in place: every output is its input
    from training.hip_tensor_env_wrappers import wrap_tensor_env

    ref = wrap_tensor_env(aligned, **kw)
    ref.use_fused = False
    with torch.cuda.stream(eng.torch_stream):
        ref.reset()
        expect = [t.clone() for t in ref.step(None)] + [ref.elapsed.clone()]
        first = ref.reset().clone()
        obs2, rew, term, trunc = (t.clone() for t in aligned.out)
        raw = aligned.raw.clone()
        elapsed = torch.zeros(n, dtype=torch.int32, device="cuda")
        eng.sync()
        torch.cuda.current_stream().synchronize()
        eng.env_wrap_step(n, obs2=obs2, rew=rew, terminated=term, truncated=trunc, obs_shift=ref._shift, obs_scale=ref._scale,
                          reward_shift=ref._reward[0], reward_scale=ref._reward[1], reward_on=True, max_episode_steps=5,
                          elapsed=elapsed, obs2_out=obs2, rew_out=rew, truncated_out=trunc)
        eng.env_wrap_reset(n, obs=raw, mask=None, obs_shift=ref._shift, obs_scale=ref._scale, elapsed=elapsed, obs_out=raw)
        eng.sync()
    _same([obs2, rew, term, trunc], expect[:4], "in place")
    assert elapsed.tolist() == [0] * n and expect[4].tolist() == [1] * n
    _same([raw], [first], "in place reset")


@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 96, 96)])         # 768 floats: one wave per row; 27 648: split over workgroups
def test_float32_frames(shared, shape):
    eng = shared.engine
    n = 2
    for per_element, offset in ((False, 0), (True, 0), (True, 1)):    # offset 1: the 4-byte path
        kw = dict(_params(shape, per_element), max_episode_steps=2, reward_shift=0.3)
        script = _script(n, shape, seed=31, offset=offset)
        want, got = _drive(eng, script, kw, False, steps=3), _drive(eng, script, kw, True, steps=3)
        for s, (x, y) in enumerate(zip(got, want)):
            _same(x, y, (per_element, s))
        assert tuple(got[0][0].shape) == (n,) + shape
        # the row's last element is the last parameter's product: nothing was left out at the tail
        last = want[1][0].reshape(n, -1)[:, -1]
        assert np.array_equal(_bits(last), _bits(got[1][0].reshape(n, -1)[:, -1]))


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_are_error_returns(shared):
    eng = shared.engine
    lib, h = eng._lib, eng._h
    n, W = 4, 8
    f = dict(dtype=torch.float32, device="cuda")
    obs2, out, shift, scale = torch.ones(n, W, **f), torch.zeros(n, W, **f), torch.zeros(W, **f), torch.full((W,), 2.0, **f)
    rew, rew_out = torch.ones(n, **f), torch.zeros(n, **f)
    term, trunc, trunc_out = (torch.zeros(n, dtype=torch.bool, device="cuda") for _ in range(3))
    elapsed = torch.zeros(n, dtype=torch.int32, device="cuda")
    host = np.zeros((n, W), np.float32)
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    calls = eng.debug_get("env_wrap_calls")

    def step(n_=n, obs2_=p(obs2), out_=p(out), rew_out_=p(rew_out), trunc_out_=p(trunc_out), reward_on=1, limit=3):
        return lib.dsact_env_wrap_step(h, n_, W, obs2_, p(rew), p(term), p(trunc), p(shift), p(scale), 0.5, 2.0, reward_on, limit,
                                       p(elapsed), out_, rew_out_, trunc_out_)

    def reset(n_=n, obs_=p(obs2), out_=p(out), elapsed_=p(elapsed)):
        return lib.dsact_env_wrap_reset(h, n_, W, obs_, None, p(shift), p(scale), elapsed_, out_)

    INVALID = -1
    refused = [
        step(obs2_=C.c_void_p(host.ctypes.data)),                    # a host pointer
        step(n_=0), step(n_=-2),
        step(out_=None), step(rew_out_=None), step(trunc_out_=None),  # an output NULL while its part is on
        step(rew_out_=p(rew_out), reward_on=0), step(limit=0),        # ... and given while its part is off
        reset(obs_=C.c_void_p(host.ctypes.data)), reset(n_=0), reset(out_=None),
    ]
    assert refused == [INVALID] * len(refused)
    assert eng.debug_get("env_wrap_calls") == calls                  # nothing was launched
    assert step() == 0 and reset() == 0                              # the handle is usable: the next calls succeed
    eng.sync()
    assert eng.debug_get("env_wrap_calls") == calls + 2
    assert torch.equal(out, torch.full((n, W), 2.0, **f)) and torch.equal(rew_out, torch.full((n,), 3.0, **f))
    assert elapsed.tolist() == [0] * n and not trunc_out.any()
    assert eng.debug_get("handoff_failures") == 0.0


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def _sampler(alg, N, S, route, graph=False, env_kw=None, **over):
    """route: 'fused' (hip_env_wrap=True), 'torch' (the same wrapper kept on the torch route)"""
    import plugin
    from synth_tensor_episodes_nolimit import SynthTensorEpisodesInplaceNoLimit, SynthTensorEpisodesNoLimit

    env = (SynthTensorEpisodesInplaceNoLimit if graph else SynthTensorEpisodesNoLimit)(N, device="cuda", **(env_kw or {}))
    kw = dict(sampler_name="hip_tensor_env_sampler", env=env, networks=alg.networks, sample_batch_size=S, seed=5, reward_scale=0.7,
              hip_env_wrap=True, **WRAP)
    if graph:
        kw["hip_graph_sample"] = True
    smp = plugin.create_sampler(**dict(kw, **over))
    if route == "torch":
        smp.env.use_fused = False
    return smp


def _take(smp, eng):
    batch, _ = smp.sample()
    eng.sync()
    return [t.detach().cpu().clone() for t in batch.device_columns]


@pytest.mark.parametrize("N", [5, 33])
def test_sampler_fused_equals_torch_route_and_the_plan(N):
    import plugin
    from synth_tensor_episodes_nolimit import plan

    S, cap, scale = 4 * N, 8 * N, 0.7
    alg, _ = make_pair(O, A, HID, 64, seed=1)
    eng = alg.engine
    buf = plugin.create_buffer(**hip_kwargs(O, A, HID, 64, buffer_max_size=cap, seed=5, hip_engine=eng))
    assert buf.engine is eng
    fused, ref = _sampler(alg, N, S, "fused"), _sampler(alg, N, S, "torch")
    k, length = [0] * N, [0] * N
    kinds = set()
    for call in range(2):
        calls = eng.debug_get("env_wrap_calls")
        batch, _ = fused.sample()
        eng.sync()
        got = [t.detach().cpu().clone() for t in batch.device_columns]
        assert fused.env.fused and eng.debug_get("env_wrap_calls") - calls == 2 * (S // N)      # one per step, one per reset
        calls = eng.debug_get("env_wrap_calls")
        want = _take(ref, eng)
        assert not ref.env.fused and eng.debug_get("env_wrap_calls") == calls
        _same(got, want, call)
        obs, act, rew, obs2, term, trunc, logp = got
        for t in range(S // N):
            for i in range(N):
                j = t * N + i
                length[i] += 1
                want_len, want_term, want_trunc = plan(i, k[i], M)
                ended = length[i] == want_len
                assert (bool(term[j]), bool(trunc[j])) == ((want_term, want_trunc) if ended else (False, False)), (call, t, i)
                # the shaped reward: (table - |a|^2 + 0.3) in fp32; the observation: ((code / 64 - 1) + 0.1) * ramp
                code = (131 * i + 71 * k[i] + 29 * length[i] + 17 * np.arange(O)) % 128
                raw = code.astype(np.float32) * np.float32(1 / 64) - np.float32(1)
                assert np.array_equal(_bits(obs2[j]), _bits((raw + np.float32(0.1)) * RAMP)), (call, t, i)
                if ended:                                            # (both fire: terminated in the limit's own step)
                    kinds.add("both" if want_term and want_len == M else "terminated" if want_term else "truncated")
                    k[i], length[i] = k[i] + 1, 0
        # the ring rows: done = terminated & ~truncated (a truncated row is stored non-terminal), reward * reward_scale
        buf.add_batch(batch)                                         # (its [S, .] buffers are valid until fused's next sample())
        eng.sync()
        rows = eng.buffer_export(call * S, S)
        assert np.array_equal(rows["done"] != 0, (term & ~trunc).numpy())
        assert np.array_equal(_bits(rows["rew"]), _bits(rew.numpy() * np.float32(scale)))
        assert np.array_equal(_bits(rows["obs2"]), _bits(obs2)) and np.array_equal(_bits(rows["obs"]), _bits(obs))
    assert kinds == ({"terminated", "truncated", "both"} if N == 33 else {"terminated", "truncated"})
    assert eng.debug_get("act_dev_syncs") == 0.0 and eng.debug_get("handoff_failures") == 0.0


def test_sampler_under_hip_graph_sample(shared):
    alg = shared
    eng = alg.engine
    N, S = 33, 4 * 33
    eager, graph = _sampler(alg, N, S, "fused"), _sampler(alg, N, S, "fused", graph=True)
    assert graph.graph_sample and graph.env.capture_safe is True
    for call in range(4):                                            # eager warm-up, capture + replay, two more replays
        _same(_take(graph, eng), _take(eager, eng), call)
    assert graph.graph_captures == 1 and graph.graph_replays == 3 and graph.env.fused
    assert torch.equal(graph.env.elapsed, eager.env.elapsed)
    assert eng.debug_get("act_dev_syncs") == 0.0 and eng.debug_get("handoff_failures") == 0.0


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def _evaluator(alg, N, E, route, graph=False, **over):
    import plugin
    from synth_tensor_episodes_nolimit import SynthTensorEpisodesInplaceNoLimit, SynthTensorEpisodesNoLimit

    env = (SynthTensorEpisodesInplaceNoLimit if graph else SynthTensorEpisodesNoLimit)(N, device="cuda")
    kw = dict(evaluator_name="hip_tensor_env_evaluator", eval_env=env, num_eval_episode=E, networks=alg.networks, hip_eval_poll_steps=4,
              hip_env_wrap=True, reward_scale=0.7, **WRAP)
    if graph:
        kw["hip_graph_eval"] = True
    ev = plugin.create_evaluator(**dict(kw, **over))
    if route == "torch":
        ev.env.use_fused = False
    return ev


def test_evaluator_routes_agree_and_follow_the_plan(shared, tmp_path):
    from synth_tensor_episodes_nolimit import plan

    alg = shared
    eng = alg.engine
    N, E = 5, 23
    runs = {}
    for name, route, graph in (("torch", "torch", False), ("eager", "fused", False), ("graph", "fused", True)):
        ev = _evaluator(alg, N, E, route, graph)
        out = []
        for it in range(3):
            tar = ev.run_evaluation(it)
            out.append((np.array([tar]), ev.returns.copy(), ev.lengths.copy(), ev.steps))
        runs[name] = (ev, out)
        assert ev.env.fused == (route == "fused")
    for name in ("eager", "graph"):
        for x, y in zip(runs[name][1], runs["torch"][1]):
            assert np.array_equal(x[0].view(np.uint64), y[0].view(np.uint64)) and np.array_equal(x[1].view(np.uint64), y[1].view(np.uint64))
            assert np.array_equal(x[2], y[2]) and x[3] == y[3], name
    ev, out = runs["graph"]
    assert ev.graph_captures == 1 and ev.graph_replays >= 2
    lengths = out[0][2]
    assert lengths.tolist() == [plan(e % N, e // N, M)[0] for e in range(E)] and lengths.max() == M and lengths.min() < M
    # returns sum the SHIFTED reward (the evaluator passes reward_shift, never reward_scale): against the bare environment's
    # evaluation on the unshifted reward -- same observations, same actions -- by 0.3 per step; a step's fp32 add rounds by at most
    # 2^-24 * 4 (|r + 0.3| < 4), five steps at most: 1.2e-6 < 1e-5
    unshaped = _evaluator(alg, N, E, "fused", reward_shift=None)
    unshaped.run_evaluation(0)
    assert np.array_equal(unshaped.lengths, lengths)
    assert np.allclose(out[0][1], unshaped.returns + 0.3 * lengths, rtol=0, atol=1e-5)
    assert np.abs(out[0][1] - unshaped.returns).min() > 0.29
    # eval_save without hip_eval_save_max_steps: the wrapper's max_episode_steps is the step bound
    saver = _evaluator(alg, N, 7, "fused", eval_save=True, save_folder=str(tmp_path))
    assert saver.save_max_steps == M
    os.makedirs(str(tmp_path / "evaluator"), exist_ok=True)
    saver.run_evaluation(0)
    assert saver.trace_dropped == 0 and len(saver.saved_files) == 7
    ep = np.load(saver.saved_files[0], allow_pickle=True).item()
    assert len(ep["reward_list"]) == int(saver.lengths[0]) and np.asarray(ep["obs_list"][0]).shape == (O,)
    assert eng.debug_get("handoff_failures") == 0.0


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_run_state_resumes_a_wrapped_sampler_bit_for_bit():
    import plugin
    from synth_tensor_humanoid_inplace import SynthTensorHumanoidInplace

    N, S = 8, 16
    kw = hip_kwargs(376, 17, HID, 64, buffer_max_size=1000, seed=5, sample_batch_size=S, strict_rng=False)
    torch.manual_seed(1)
    alg = plugin.create_alg(**kw)
    eng = alg.engine

    def make():
        env = SynthTensorHumanoidInplace(N, device="cuda", seed=4, episode_limit=1000)
        return plugin.create_sampler(**dict(kw, sampler_name="hip_tensor_env_sampler", env=env, networks=alg.networks, hip_env_wrap=True,
                                            max_episode_steps=7, reward_shift=0.3, obs_scale=0.5))

    a = make()
    for _ in range(2):
        _take(a, eng)
    sd = a.run_state()                                               # 4 lockstep steps in: elapsed is 4 (or less after a restart)
    assert sd["env"]["format"].startswith("dsact-tensor-env-wrap-state") and 0 < int(sd["env"]["elapsed"].max()) < 7
    b = make()
    b.load_run_state(sd)
    assert torch.equal(a.env.elapsed, b.env.elapsed) and b.env.fused
    for call in range(2):                                            # the limit fires inside these (steps 5 .. 8)
        x, y = _take(a, eng), _take(b, eng)
        _same(x, y, call)
    assert bool(x[5].any()) or bool(y[5].any())


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_serial_trainer_ends_bitwise_equal_on_both_routes(tmp_path):
    import plugin
    from synth_tensor_episodes_nolimit import SynthTensorEpisodesInplaceNoLimit
    from training.hip_trainer import TB, HipOffSerialTrainer, read_scalars

    N, S, iters, cap, warm, every = 32, 64, 60, 4000, 128, 20
    finals, tars = [], []
    for fused in (False, True):
        folder = str(tmp_path / ("fused" if fused else "torch"))
        kw = hip_kwargs(O, A, HID, 64, buffer_max_size=cap, buffer_warm_size=warm, seed=3, sample_batch_size=S,
                        sample_interval=1, max_iteration=iters, log_save_interval=20, apprfunc_save_interval=100000,
                        eval_interval=every, save_folder=folder, ini_network_dir=None, strict_rng=False, hip_device_indices=True,
                        sampler_name="hip_tensor_env_sampler", evaluator_name="hip_tensor_env_evaluator", num_eval_episode=40,
                        hip_graph_sample=True, hip_graph_eval=True, hip_env_wrap=True, reward_scale=0.7, **WRAP)
        torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
        alg = plugin.create_alg(**kw)
        buf = plugin.create_buffer(**kw)
        smp = plugin.create_sampler(env=SynthTensorEpisodesInplaceNoLimit(N, device="cuda"), **kw)
        ev = plugin.create_evaluator(eval_env=SynthTensorEpisodesInplaceNoLimit(33, device="cuda"), **kw)
        if not fused:
            smp.env.use_fused = ev.env.use_fused = False
        tr = plugin.create_trainer(alg, smp, buf, ev, **kw)
        assert type(tr) is HipOffSerialTrainer
        tr.train()
        e = alg.engine
        e.sync()
        assert smp.env.fused == fused and ev.env.fused == fused
        assert (e.debug_get("env_wrap_calls") > 0) == fused
        assert e.debug_get("handoff_failures") == 0.0 and e.debug_get("act_dev_syncs") == 0.0
        assert smp.graph_captures == 1 and smp.graph_replays >= 2 and ev.graph_captures == 1
        logged = read_scalars(folder)[TB["tar_iter"]]
        tars.append([float(y) for y in logged["y"]])
        finals.append((e.buffer_digest(), buf.size, buf.ptr, e.online.cpu().clone(), e.target.cpu().clone(), e.adam_m.cpu().clone(),
                       e.adam_v.cpu().clone()))
    assert np.array_equal(np.array(tars[0]).view(np.uint64), np.array(tars[1]).view(np.uint64)) and len(tars[0]) == 3
    assert finals[0][:3] == finals[1][:3]
    for x, y in zip(finals[0][3:], finals[1][3:]):
        assert torch.equal(x, y)
