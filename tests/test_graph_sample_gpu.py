"""A sample() as one captured graph on the GPU (csrc/dsact_act_batch.h counted forms, k_counter_set / k_counter_add / k_step_rows,
training/hip_tensor_sampler.py with hip_graph_sample=True). Everything is compared BITWISE: the captured
route computes what the eager route computes, with fewer host calls.

  1. dsact_act_sample_device_counted(counter = c, offset = t) == dsact_act_sample_device(eps = NULL, step = c + t), across the
     32-bit carry of the counter, over two chunks, with every exploration-noise form; counter_add / counter_read;
  2. a sampler with the kwarg on the in-place fixture == an eager sampler on the plain fixture over eager call, capture and
     replays, restarts inside the replays, without and with per-dimension noise_params;
  3. a replay acts with the weights that are in the arena when it runs;
  4. act_step assigned between replays (to just below 2^32);
  5. HipOffSerialTrainer ends bitwise equal on both routes, K = 1 and 8;
  6. episode_statistics() is the same on both routes;
  7. run_state() / load_run_state() into a fresh sampler (which warms up and captures again);
  8. dsact_step_rows_device == the four torch copies and the `|`, and touches nothing around its slots.
"""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

O, A, HID = 376, 17, (64, 64)          # the fixture's shapes
N, S = 8, 32                           # four lockstep steps per sample()
# six sample() calls are 24 lockstep steps; an episode of environment i lasts at most its limit 3 + i, so it ends at least
# 24 // (3 + i) times: 8 + 6 + 4 + 4 + 3 + 3 + 2 + 2
MIN_EPISODES = sum(6 * (S // N) // (3 + i) for i in range(N))
PER_DIM = {"mean": np.linspace(-0.05, 0.05, A).tolist(), "std": np.linspace(0.02, 0.2, A).tolist()}


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.uint8 if t.dtype == torch.bool else np.uint32 if t.dtype == torch.float32 else t.numpy().dtype)


def _alg(obs=O, act=A, seed=1, **over):
    import plugin

    kw = hip_kwargs(obs, act, HID, 64, buffer_max_size=4000, seed=5, sample_batch_size=S, strict_rng=False, **over)
    torch.manual_seed(seed)
    return plugin.create_alg(**kw), kw


def _sampler(alg, kw, graph, limit=None, **over):
    import plugin
    from synth_tensor_humanoid import SynthTensorHumanoid
    from synth_tensor_humanoid_inplace import SynthTensorHumanoidInplace

    limit = torch.arange(3, 3 + N) if limit is None else limit                       # 3 .. 10: restarts fall inside every call
    env = (SynthTensorHumanoidInplace if graph else SynthTensorHumanoid)(N, device="cuda", seed=4, episode_limit=limit)
    more = dict(hip_graph_sample=True) if graph else {}
    more.update(over)
    return plugin.create_sampler(**dict(kw, sampler_name="hip_tensor_env_sampler", env=env, networks=alg.networks, **more))


def _take(smp, eng):
    """one sample(): the seven tensors of the batch as CPU clones"""
    batch, _ = smp.sample()
    eng.sync()
    return [t.detach().cpu().clone() for t in batch.device_columns]


def _same(x, y, what):
    for k, (u, v) in enumerate(zip(x, y)):
        assert u.dtype == v.dtype and np.array_equal(_bits(u), _bits(v)), (what, k)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [None, "shared", "per_dim"])
def test_counted_call_is_bitwise_the_stepped_call(noise):
    Os, As = 17, 6
    alg, _ = _alg(Os, As)
    e = alg.engine
    e.set_act_rng(0x1234567887654321)
    if noise == "shared":
        e.set_explore_noise(0.01, 0.1)
    elif noise == "per_dim":
        e.set_explore_noise(np.linspace(-0.05, 0.05, As), np.linspace(0.02, 0.2, As))
    g = torch.Generator(device="cuda").manual_seed(2)
    for n in (1, 33, 1030):                                             # 1030: two chunks -- the second starts at row0 = 1024
        obs = 2.0 * torch.randn(n, Os, device="cuda", generator=g)
        out = [[torch.empty(n, As, device="cuda"), torch.empty(n, As, device="cuda"), torch.empty(n, device="cuda")] for _ in range(2)]
        torch.cuda.synchronize()
        calls = e.debug_get("act_dev_calls")
        for c in (0, 2 ** 32 - 2):                                      # t = 2, 3 carry into the high word
            e.act_counter_set(c)
            for t in range(4):
                e.act_sample_device_counted(obs, t, *out[0])
                e.act_sample_device(obs, None, c + t, *out[1])
                e.sync()
                for k, name in enumerate(("action", "clipped", "logp")):
                    assert np.array_equal(_bits(out[0][k]), _bits(out[1][k])), (n, c, t, name)
            assert e.act_counter_read() == c                            # the acting calls read the word, they never move it
            if c:                                                       # ... and the high word is part of the key
                e.act_sample_device(obs, None, (c + 3) & 0xFFFFFFFF, *out[1])
                e.sync()
                assert not np.array_equal(_bits(out[0][0]), _bits(out[1][0])), n
        assert e.debug_get("act_dev_calls") - calls == (2 * 4 * 2 + 1) * ((n + 1023) // 1024)
    for c in (0, 7, 2 ** 32 - 2, 2 ** 64 - 3):
        e.act_counter_set(c)
        e.act_counter_add(5)
        assert e.act_counter_read() == (c + 5) % 2 ** 64
    e.act_counter_add(-2)
    assert e.act_counter_read() == 0
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


def test_counted_call_refusals():
    from dsact._ffi import DsactError

    alg, _ = _alg(17, 6)
    e = alg.engine
    e.set_act_rng(3)
    obs = torch.zeros(4, 17, device="cuda")
    act, clip, lp = torch.empty(4, 6, device="cuda"), torch.empty(4, 6, device="cuda"), torch.empty(4, device="cuda")
    torch.cuda.synchronize()
    for call in (lambda: e.act_sample_device_counted(obs, 0, act, clip, lp), lambda: e.act_counter_add(1), e.act_counter_read):
        with pytest.raises(DsactError, match="E_STATE.*dsact_act_counter_set"):
            call()
    e.act_counter_set(1)
    g = torch.cuda.CUDAGraph()
    refused = []
    with torch.cuda.graph(g, stream=e.torch_stream, capture_error_mode="relaxed"):
        for call in (lambda: e.act_counter_set(2), e.act_counter_read,
                     lambda: e.act_sample_device_counted(obs, 0, act, clip, lp)):   # (no eager acting call yet: nothing allocated)
            try:
                call()
                refused.append(None)
            except DsactError as ex:
                refused.append(str(ex))
    del g
    assert all(r is not None and "E_STATE" in r and "capture" in r for r in refused), refused
    e.act_sample_device_counted(obs, 0, act, clip, lp)                  # outside: accepted, and the handle is usable
    assert e.act_counter_read() == 1
    with pytest.raises(ValueError):
        e.act_sample_device_counted(obs.cpu(), 0, act, clip, lp)


# ---- 2, 6 ----------------------------------------------------------------------------------------------------------------------
def _pair(noise=None, **over):
    (alg_e, kw), (alg_g, _) = _alg(), _alg()
    assert torch.equal(alg_e.engine.online, alg_g.engine.online)
    extra = dict(noise_params=noise) if noise is not None else {}
    extra.update(over)
    return (alg_e, _sampler(alg_e, kw, False, **extra)), (alg_g, _sampler(alg_g, kw, True, **extra))


def _state_equal(se, sg, eg):
    eg.sync()
    assert np.array_equal(_bits(se._obs), _bits(sg._obs))
    assert se.act_step == sg.act_step == eg.act_counter_read()
    assert torch.equal(se.env.pos, sg.env.pos) and torch.equal(se.env.t, sg.env.t)


@pytest.mark.parametrize("noise", [None, PER_DIM])
def test_graph_route_is_bitwise_the_eager_route(noise):
    (alg_e, se), (alg_g, sg) = _pair(noise)
    ee, eg = alg_e.engine, alg_g.engine
    ended = 0
    for call in range(6):                                               # eager, capture (+ its replay), four replays
        be, bg = _take(se, ee), _take(sg, eg)
        _same(be, bg, call)
        assert bool((be[4] | be[5]).any())                              # environments restarted inside this call (limit 3 < S / N)
        ended += int((be[4] | be[5]).sum())
        assert sg.graph_captures == min(call, 1) and sg.graph_replays == call
    assert ended >= MIN_EPISODES
    _state_equal(se, sg, eg)
    assert sg.act_step == 6 * S // N and sg.graph_captures == 1 and sg.graph_replays == 5
    assert se.graph_captures == 0 and se.graph_replays == 0
    assert eg.debug_get("act_dev_syncs") == 0.0 and eg.debug_get("handoff_failures") == 0.0
    # the replays made no library call per step: the eager and the capturing call issued all there are
    assert eg.debug_get("act_dev_calls") == 2 * S // N and eg.debug_get("step_rows_calls") == 2 * S // N
    assert ee.debug_get("act_dev_calls") == 6 * S // N and ee.debug_get("step_rows_calls") == 0.0


def test_episode_statistics_are_the_same_on_both_routes():
    (alg_e, se), (alg_g, sg) = _pair(hip_episode_stats=True)
    for call in range(6):
        _same(_take(se, alg_e.engine), _take(sg, alg_g.engine), call)
    a, b = se.episode_statistics(), sg.episode_statistics()
    assert a["episodes"] == b["episodes"] >= MIN_EPISODES
    for k in ("terminated_share", "return_mean", "return_min", "return_max", "length_mean"):
        assert a[k] == b[k], k
    for k, v in a["rows"].items():
        assert np.array_equal(v, b["rows"][k]), k
    assert alg_g.engine.debug_get("track_commit_calls") == 6.0           # one per sample(), behind the replay


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_a_replay_reads_the_live_weights():
    alg, kw = _alg()
    e = alg.engine
    smp = _sampler(alg, kw, True)
    for _ in range(3):
        _take(smp, e)
    assert smp.graph_replays == 2
    out = [[torch.empty(N, A, device="cuda"), torch.empty(N, A, device="cuda"), torch.empty(N, device="cuda")] for _ in range(2)]
    with torch.cuda.stream(e.torch_stream), torch.no_grad():
        obs = smp._obs.clone()
        e.act_sample_device(obs, None, smp.act_step, *out[0])           # what the old weights would do at this step
        for p in alg.networks.policy.parameters():                      # the arena, written in place in stream order
            p.mul_(1.25)
    if hasattr(e, "policy_dirty"):
        e.policy_dirty()
    step = smp.act_step
    got = _take(smp, e)                                                 # a replay: nothing of it is issued anew
    assert smp.graph_replays == 3 and smp.graph_captures == 1
    with torch.cuda.stream(e.torch_stream):
        e.act_sample_device(obs, None, step, *out[1])
    e.sync()
    assert np.array_equal(_bits(got[0][:N]), _bits(obs))
    assert np.array_equal(_bits(got[1][:N]), _bits(out[1][0])) and np.array_equal(_bits(got[6][:N]), _bits(out[1][2]))
    assert not np.array_equal(_bits(out[0][0]), _bits(out[1][0]))       # the weights did move the action


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_act_step_assigned_between_replays():
    (alg_e, se), (alg_g, sg) = _pair()
    for call in range(3):
        _same(_take(se, alg_e.engine), _take(sg, alg_g.engine), call)
    se.act_step = sg.act_step = 2 ** 32 - 2
    assert sg.act_step == 2 ** 32 - 2 and alg_g.engine.act_counter_read() == 2 ** 32 - 2
    for call in range(2):                                               # steps 2^32 - 2 .. 2^32 + 5: across the carry
        _same(_take(se, alg_e.engine), _take(sg, alg_g.engine), ("assigned", call))
    _state_equal(se, sg, alg_g.engine)
    assert sg.act_step == 2 ** 32 - 2 + 2 * S // N and sg.graph_captures == 1 and sg.graph_replays == 4


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
def test_serial_trainer_ends_bitwise_equal_on_both_routes(tmp_path, K):
    import plugin
    from training.hip_trainer import HipOffSerialTrainer

    iters, cap, warm = 40, 2000, 64
    finals = []
    for graph in (False, True):
        kw = hip_kwargs(O, A, HID, 64, buffer_max_size=cap, buffer_warm_size=warm, seed=3, sample_batch_size=S, sample_interval=K,
                        max_iteration=iters, log_save_interval=20, apprfunc_save_interval=100000, eval_interval=100000,
                        save_folder=str(tmp_path / ("graph" if graph else "eager")), ini_network_dir=None, strict_rng=False,
                        hip_device_indices=True, reward_scale=0.25, sampler_name="hip_tensor_env_sampler")
        torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
        alg = plugin.create_alg(**kw)
        buf = plugin.create_buffer(**kw)
        smp = _sampler(alg, kw, graph)
        tr = plugin.create_trainer(alg, smp, buf, None, **kw)
        assert type(tr) is HipOffSerialTrainer
        tr.train()
        e = alg.engine
        e.sync()
        n_samples = warm // S * S + (iters + K - 1) // K * S
        assert smp.get_total_sample_number() == n_samples and smp.act_step == n_samples // N
        assert e.debug_get("handoff_failures") == 0.0 and e.debug_get("act_dev_syncs") == 0.0
        if graph:
            assert smp.graph_captures == 1 and smp.graph_replays == n_samples // S - 1 and e.act_counter_read() == smp.act_step
        finals.append((e.buffer_digest(), buf.size, buf.ptr, e.online.cpu().clone(), e.target.cpu().clone(), e.adam_m.cpu().clone(),
                       e.adam_v.cpu().clone()))
    assert finals[0][:3] == finals[1][:3]
    for x, y in zip(finals[0][3:], finals[1][3:]):
        assert torch.equal(x, y)


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_resume_into_a_fresh_sampler():
    alg, kw = _alg()
    e = alg.engine
    first = _sampler(alg, kw, True, noise_params=PER_DIM)
    for _ in range(3):
        _take(first, e)
    sd = first.run_state()
    assert sd["act_step"] == 3 * S // N and sd["format"] == first.RUN_STATE_FORMAT
    want = [_take(first, e), _take(first, e)]
    fresh = _sampler(alg, kw, True, noise_params=PER_DIM)               # the same engine: its counter is written anew
    fresh.load_run_state(sd)
    assert fresh.act_step == 3 * S // N and e.act_counter_read() == 3 * S // N
    for k in range(2):                                                  # an eager call, then capture + replay: the bits do not care
        _same(want[k], _take(fresh, e), ("resumed", k))
    assert fresh.graph_captures == 1 and fresh.graph_replays == 1 and fresh.act_step == 5 * S // N == e.act_counter_read()


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [376, 17])                                # 16 bytes per lane / 4 bytes per lane
def test_step_rows_equal_the_torch_copies(W):
    alg, _ = _alg(17, 6)
    e = alg.engine
    g = torch.Generator(device="cuda").manual_seed(9)
    for n in (1, 5, 1030):
        rows = 3 * n                                                    # the slot is rows [n, 2n): bytes on both sides of it
        obs2, rew = torch.randn(n, W, device="cuda", generator=g), torch.randn(n, device="cuda", generator=g)
        term, trunc = (torch.rand(n, device="cuda", generator=g) < 0.3 for _ in range(2))
        got = [torch.full((rows, W), 7.5, device="cuda"), torch.full((rows,), -3.25, device="cuda"),
               torch.zeros(rows, dtype=torch.bool, device="cuda"), torch.ones(rows, dtype=torch.bool, device="cuda")]
        want = [t.clone() for t in got]
        ended = torch.zeros(n, dtype=torch.bool, device="cuda")
        for dst, src in zip(want, (obs2, rew, term, trunc)):
            dst[n:2 * n].copy_(src)
        torch.cuda.synchronize()
        calls = e.debug_get("step_rows_calls")
        e.step_rows_device(obs2, rew, term, trunc, *(t[n:2 * n] for t in got), ended)
        e.sync()
        assert e.debug_get("step_rows_calls") - calls == 1
        for k, (u, v) in enumerate(zip(got, want)):
            assert np.array_equal(_bits(u), _bits(v)), (n, k)
        assert np.array_equal(_bits(ended), _bits(term | trunc)), n
        if n > 1:
            assert bool(ended.any()) and not bool(ended.all())
    assert e.debug_get("act_dev_syncs") == 0.0
    with pytest.raises(ValueError):
        e.step_rows_device(obs2.t().contiguous().t(), rew, term, trunc, *(t[n:2 * n] for t in got), ended)   # not contiguous
