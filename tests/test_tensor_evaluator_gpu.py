"""Device-resident evaluation on the GPU (csrc/dsact_act_batch.h <kMode, kDev> form, k_eval_commit, dsact_act_mode_device /
dsact_eval_*, training/hip_tensor_evaluator.py):

  1. act_mode_device equals act_mode_batch's GPU route bit for bit;
  2. k_eval_commit alone, driven with scripted rewards and flags, equals the NumPy restatement of
     tests/test_tensor_evaluator_host.py step by step;
  3. HipTensorEnvEvaluator.run_evaluation on tests/envs/synth_tensor_episodes.py equals a restatement (act_mode_batch per step +
     NumPy fp64 bookkeeping + the same environment class), for every poll period;
  4. an evaluation leaves the training state and the generators alone;
  5. HipOffSerialTrainer runs with the tensor sampler plus this evaluator; two runs from the same seeds end bitwise equal;
  6. refusals on the real engine leave the handle usable.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs
from test_hip_parity import make_pair
from test_tensor_evaluator_host import FakeEngine

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

O, A, HID = 17, 6, (64, 64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o,a,hid,B,sizes,over", [
    (O, A, HID, 64, (1, 33, 256, 1030), {}),
    (24, 6, HID, 64, (1, 33, 256, 1030), {"policy_std_type": "mlp_separated"}),
    (24, 6, HID, 64, (1, 33, 256, 1030), {"policy_output_activation": "tanh", "value_output_activation": "tanh"}),
    (24, 6, HID, 64, (1, 33, 256, 1030), {"policy_act_distribution": "GaussDistribution"}),
    (376, 17, (256, 256, 256), 256, (33,), {}),                                                    # the BASELINE policy
])
def test_acting_is_bitwise_the_batch_calls_gpu_route(o, a, hid, B, sizes, over):
    alg, _ = make_pair(o, a, hid, B, seed=61, **over)
    e = alg.engine
    rng = np.random.default_rng(3)
    for n in sizes:
        obs = torch.from_numpy((10.0 * rng.standard_normal((n, o))).astype(np.float32)).cuda()
        act = torch.full((n, a), float("nan"), device="cuda")
        torch.cuda.synchronize()                     # the inputs were produced on torch's stream; the call runs on the engine's
        calls, mode_calls = e.debug_get("act_mode_dev_calls"), e.debug_get("act_mode_calls")
        e.act_mode_device(obs, act)
        assert e.debug_get("act_mode_dev_calls") - calls == (n + 1023) // 1024
        e.sync()
        got = act.cpu().numpy()
        want = e.act_mode_batch(obs)                 # a CUDA tensor: the batched GPU forward whatever n is
        assert e.debug_get("act_mode_calls") - mode_calls == (n + 1023) // 1024
        assert np.array_equal(_bits(got), _bits(want)), (n, np.abs(got - want).max())
        assert np.abs(got).max() <= np.float32(0.4)
        if over.get("policy_act_distribution") == "GaussDistribution":
            assert (np.abs(got) == np.float32(0.4)).any()      # the clamp of the plain Gaussian's mode had something to do
    assert e.debug_get("act_dev_syncs") == 0.0


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_engine():
    alg, _ = make_pair(O, A, HID, 64, seed=4)
    return alg


@pytest.mark.parametrize("N", [5, 33, 300])
def test_bookkeeping_equals_the_restatement_step_by_step(small_engine, N):
    from dsact._ffi import DsactError

    e = small_engine.engine
    T = 400
    for E in (3, N, 4 * N + 1):
        g = torch.Generator().manual_seed(1000 * N + E)
        # rewards whose fp32 running sum would round: the fp64 sum in step order is the only value that matches
        rew = (torch.randn(T, N, generator=g) * torch.tensor(10.0) ** torch.randint(-3, 4, (T, N), generator=g).float()).contiguous()
        term, trunc = torch.rand(T, N, generator=g) < 0.2, torch.rand(T, N, generator=g) < 0.2
        term[:, 1] = trunc[:, 1] = True                                         # a row whose every episode has length 1
        term[:2, 0] = trunc[:2, 0] = False                                      # ... and an episode longer than that
        d_rew, d_term, d_trunc = rew.cuda(), term.cuda(), trunc.cuda()
        d_ended = torch.zeros(T, N, dtype=torch.bool, device="cuda")
        torch.cuda.synchronize()
        ref = FakeEngine()
        ref.eval_begin(N, E)
        e.eval_begin(N, E)
        commits, syncs = e.debug_get("eval_commit_calls"), e.debug_get("act_dev_syncs")
        ended_ref = torch.zeros(T, N, dtype=torch.bool)
        t = 0
        while ref.remaining:
            assert t < T
            if t == 0:
                with pytest.raises(DsactError, match="E_STATE"):
                    e.eval_read(E)                                              # before the end
            e.eval_commit(d_rew[t], d_term[t], d_trunc[t], d_ended[t])
            ref.eval_commit(rew[t], term[t], trunc[t], ended_ref[t])
            assert e.eval_poll() == ref.remaining, (E, t)
            t += 1
        assert (term[:t] & trunc[:t]).any() and e.debug_get("eval_commit_calls") - commits == t
        assert e.debug_get("act_dev_syncs") == syncs
        # rows without an episode: commits past the end count nothing and still report the ends
        e.eval_commit(d_rew[t], d_term[t], d_trunc[t], d_ended[t])
        ref.eval_commit(rew[t], term[t], trunc[t], ended_ref[t])
        assert e.eval_poll() == 0
        returns, lengths = e.eval_read(E)
        assert returns.dtype == np.float64 and lengths.dtype == np.int32
        assert np.array_equal(_bits(returns), _bits(ref.returns)), (N, E)
        assert np.array_equal(lengths, ref.lengths), (N, E)
        assert torch.equal(d_ended[:t + 1].cpu(), ended_ref[:t + 1]) and torch.equal(ended_ref[:t + 1], (term | trunc)[:t + 1])
        assert lengths.min() == 1 and lengths.max() > 1 and lengths.sum() >= t


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def _restatement(e, N, E):
    """act_mode_batch per lockstep step over all rows, NumPy fp64 bookkeeping, the same environment class"""
    from synth_tensor_episodes import SynthTensorEpisodes

    env = SynthTensorEpisodes(N, device="cuda")
    book = FakeEngine()
    book.eval_begin(N, E)
    obs = env.reset()
    ended = torch.zeros(N, dtype=torch.bool)
    steps = 0
    while book.remaining:
        act = torch.from_numpy(e.act_mode_batch(obs.contiguous())).cuda()
        obs2, rew, term, trunc = env.step(act)
        book.eval_commit(rew.cpu(), term.cpu(), trunc.cpu(), ended)
        obs = env.reset(ended.cuda())
        steps += 1
    return book.returns, book.lengths, steps


@pytest.mark.parametrize("N,E", [(5, 7), (33, 40), (5, 70), (5, 3)])
def test_whole_evaluator_equals_the_restatement(small_engine, N, E):
    import plugin
    from synth_tensor_episodes import SynthTensorEpisodes, episode_plan
    from training.hip_tensor_evaluator import HipTensorEnvEvaluator

    alg = small_engine
    e = alg.engine
    want_ret, want_len, want_steps = _restatement(e, N, E)
    plans = [episode_plan(k % N, k // N) for k in range(E)]
    assert [int(n) for n in want_len] == [p[0] for p in plans]
    # what this case is here for, by the fixture's arithmetic
    kinds = {(te, tr) for _, te, tr in plans}
    assert (True, False) in kinds and (False, True) in kinds
    if (N, E) in ((33, 40), (5, 70)):
        assert (True, True) in kinds and 1 in want_len
    assert (N, E) != (5, 70) or E // N > 3
    assert (N, E) != (5, 3) or E < N
    for P in (1, 7, 64):
        ev = plugin.create_evaluator(evaluator_name="hip_tensor_env_evaluator", eval_env=SynthTensorEpisodes(N, device="cuda"),
                                     num_eval_episode=E, networks=alg.networks, hip_eval_poll_steps=P)
        assert type(ev) is HipTensorEnvEvaluator
        for again in range(2):                                                  # begin and reset re-initialise
            polls, syncs = e.debug_get("eval_polls"), e.debug_get("act_dev_syncs")
            tar = ev.run_evaluation(again)
            assert np.array_equal(_bits(ev.returns), _bits(want_ret)), (P, again)
            assert np.array_equal(ev.lengths, want_len), (P, again)
            assert np.array_equal(_bits(np.array([tar])), _bits(np.array([np.mean(want_ret)])))
            assert ev.steps == -(-want_steps // P) * P
            assert e.debug_get("eval_polls") - polls == -(-ev.steps // P)
            assert e.debug_get("act_dev_syncs") == syncs == 0.0
    # the actions reach the returns: every one is below the sum of its reward-table entries by the |a|^2 terms
    table = [sum(((37 * (k % N) + 101 * t + 11) % 64) / 16 - 2 for t in range(1, plans[k][0] + 1)) for k in range(E)]
    assert np.isfinite(want_ret).all() and (want_ret < np.array(table) - 1e-3).all()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_training_state_is_untouched(small_engine):
    import plugin
    from synth_tensor_episodes import SynthTensorEpisodes

    alg = small_engine
    e = alg.engine
    arenas = lambda: [t.clone() for t in (e.online, e.target, e.adam_m, e.adam_v)]
    e.sync()
    torch.cuda.synchronize()
    before, state = arenas(), e.get_state()
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state())
    ev = plugin.create_evaluator(evaluator_name="hip_tensor_env_evaluator", eval_env=SynthTensorEpisodes(33, device="cuda"),
                                 num_eval_episode=40, networks=alg.networks)
    assert np.isfinite(ev.run_evaluation(0))
    e.sync()
    for x, y in zip(before, arenas()):
        assert torch.equal(x, y)
    assert e.get_state() == state
    assert torch.equal(rng[0], torch.get_rng_state()) and torch.equal(rng[1], torch.cuda.get_rng_state())
    now = np.random.get_state()
    assert rng[2][0] == now[0] and np.array_equal(rng[2][1], now[1]) and rng[2][2:] == now[2:]


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_serial_trainer_runs_with_sampler_and_evaluator(tmp_path):
    import plugin
    from synth_tensor_episodes import SynthTensorEpisodes
    from training.hip_tensor_evaluator import HipTensorEnvEvaluator
    from training.hip_trainer import TB, HipOffSerialTrainer, read_scalars

    N, S, iters, cap, warm, every = 32, 64, 200, 4000, 128, 50
    finals, tars = [], []
    for run in range(2):
        folder = str(tmp_path / ("run%d" % run))
        kw = hip_kwargs(O, A, HID, 64, buffer_max_size=cap, buffer_warm_size=warm, seed=3, sample_batch_size=S,
                        sample_interval=1, max_iteration=iters, log_save_interval=40, apprfunc_save_interval=100000,
                        eval_interval=every, save_folder=folder, ini_network_dir=None, strict_rng=False, hip_device_indices=True,
                        sampler_name="hip_tensor_env_sampler", evaluator_name="hip_tensor_env_evaluator", num_eval_episode=40)
        torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
        alg = plugin.create_alg(**kw)
        buf = plugin.create_buffer(**kw)
        smp = plugin.create_sampler(env=SynthTensorEpisodes(N, device="cuda"), **kw)
        ev = plugin.create_evaluator(eval_env=SynthTensorEpisodes(33, device="cuda"), **kw)   # its own instance
        assert type(ev) is HipTensorEnvEvaluator
        seen = []
        run_evaluation = ev.run_evaluation
        ev.run_evaluation = lambda it: (seen.append((it, run_evaluation(it), ev.returns.copy(), ev.lengths.copy())), seen[-1][1])[1]
        tr = plugin.create_trainer(alg, smp, buf, ev, **kw)
        assert type(tr) is HipOffSerialTrainer
        tr.train()
        e = alg.engine
        e.sync()
        assert [s[0] for s in seen] == list(range(0, iters, every)) and len(seen) >= 3
        assert all(np.isfinite(s[1]) and np.isfinite(s[2]).all() for s in seen)
        assert e.debug_get("handoff_failures") == 0.0 and e.debug_get("act_dev_syncs") == 0.0
        assert len(read_scalars(folder)[TB["tar_iter"]]["y"]) == len(seen)
        assert len({s[1] for s in seen}) > 1                                     # the policy moved between evaluations
        assert torch.isfinite(e.online).all()
        finals.append((e.online.cpu().clone(), e.target.cpu().clone(), e.adam_m.cpu().clone()))
        tars.append(seen)
    for x, y in zip(*finals):
        assert torch.equal(x, y)
    for s0, s1 in zip(*tars):
        assert _bits(np.array([s0[1]])) == _bits(np.array([s1[1]])) and np.array_equal(_bits(s0[2]), _bits(s1[2]))
        assert np.array_equal(s0[3], s1[3])


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from dsact._ffi import DsactError

    alg, _ = make_pair(O, A, HID, 64, seed=4)       # a fresh handle: no dsact_eval_begin yet
    e = alg.engine
    n = 8
    f = lambda *s: torch.zeros(*s, device="cuda")
    obs, act, rew = f(n, O), f(n, A), f(n)
    flags, ended = torch.zeros(n, dtype=torch.bool, device="cuda"), torch.zeros(n, dtype=torch.bool, device="cuda")
    rew2, set_flags = rew + 1.5, ~flags
    torch.cuda.synchronize()
    with pytest.raises(DsactError, match="E_STATE.*before dsact_eval_begin"):
        e.eval_commit(rew, flags, flags, ended)
    with pytest.raises(DsactError, match="E_STATE"):
        e.eval_poll()
    with pytest.raises(DsactError, match="E_INVALID"):
        e.eval_begin(0, 4)
    with pytest.raises(DsactError, match="E_INVALID"):
        e.eval_begin(4, 0)
    # host pointers (pageable and pinned) at the C-ABI itself: the Python wrapper would refuse them first
    h_obs, h_out = np.zeros((n, O), np.float32), np.zeros((n, A), np.float32)
    pinned = torch.zeros(n, O).pin_memory()
    P = lambda t: C.c_void_p(t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr())
    lib, h = e._lib, e._h
    for bad_obs in (h_obs, pinned):
        assert lib.dsact_act_mode_device(h, P(bad_obs), n, P(act)) == -1
        assert b"device pointers" in lib.dsact_last_error(h)
    assert lib.dsact_act_mode_device(h, P(obs), n, P(h_out)) == -1
    e.eval_begin(n, 4)
    h_rew, h_flag = np.zeros(n, np.float32), np.zeros(n, np.uint8)
    for args in ((h_rew, flags, flags, ended), (rew, h_flag, flags, ended), (rew, flags, h_flag, ended), (rew, flags, flags, h_flag)):
        assert lib.dsact_eval_commit(h, *[P(x) for x in args]) == -1
        assert b"device pointers" in lib.dsact_last_error(h)
    assert e.eval_poll() == 4 and e.debug_get("eval_commit_calls") == 0.0
    with pytest.raises(ValueError, match="obs must be a torch tensor on"):
        e.act_mode_device(torch.zeros(n, O), act)
    with pytest.raises(ValueError, match="dtype"):
        e.eval_commit(rew.double(), flags, flags, ended)
    with pytest.raises(ValueError, match="shape"):
        e.eval_commit(f(n + 1), flags, flags, ended)
    # ... and the handle works
    e.act_mode_device(obs, act)
    e.eval_commit(rew2, set_flags, flags, ended)
    assert e.eval_poll() == 0 and bool(ended.all())
    returns, lengths = e.eval_read(4)
    assert returns.tolist() == [1.5] * 4 and lengths.tolist() == [1] * 4
    assert torch.isfinite(act).all() and e.debug_get("act_dev_syncs") == 0.0
    assert np.array_equal(act.cpu().numpy(), e.act_mode_batch(obs))


def test_cnn_handles_are_refused():
    from dsact._ffi import DsactError
    from test_hip_groups import _family_alg

    n, o, a = 4, 3 * 96 * 96, 3
    e = _family_alg("v2_cnn", 16, seed=4)[0].engine
    obs, act = torch.zeros(n, o, device="cuda"), torch.zeros(n, a, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(DsactError, match="E_INVALID.*serves MLP policies"):
        e.act_mode_device(obs, act)
    got = e.act_mode_batch(obs.cpu().numpy())            # the handle's own route still works
    assert got.shape == (n, a) and np.isfinite(got).all()
