"""The tensor evaluator's poll windows as one captured graph on the GPU (dsact_act_mode_device / dsact_eval_commit under stream
capture, training/hip_tensor_evaluator.py with hip_graph_eval=True). Everything is compared BITWISE with the
eager evaluator: both routes run the same kernels on the same inputs.

  1. a hip_graph_eval evaluator on the in-place fixture == an eager evaluator on the plain fixture, over eager window, capture
     and replays, for every poll period and with two acting chunks per step; on that route the commit and the acting call read the
     environment's tensors in place;
  2. a replay acts with the weights that are in the arena when it runs;
  3. hip_eval_max_steps off the window grid: the remainder runs eagerly, the error leaves the handle idle and usable;
  4. another evaluator's larger dsact_eval_begin reallocates the bookkeeping: the graph is captured again;
  5. the library's rules under capture, each refusal leaving the handle usable;
  6. three captured evaluations leave the training state and the generators alone;
  7. HipOffSerialTrainer with both captured routes ends bitwise equal to the run with neither.
"""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs, synth_batch
from test_hip_parity import make_pair

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

O, A, HID = 17, 6, (64, 64)
NAME = "hip_tensor_env_evaluator"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _evaluator(alg, N, E, graph, **over):
    import plugin
    from synth_tensor_episodes import SynthTensorEpisodes
    from synth_tensor_episodes_inplace import SynthTensorEpisodesInplace

    env = (SynthTensorEpisodesInplace if graph else SynthTensorEpisodes)(N, device="cuda")
    more = dict(hip_graph_eval=True) if graph else {}
    more.update(over)
    return plugin.create_evaluator(evaluator_name=NAME, eval_env=env, num_eval_episode=E, networks=alg.networks, **more)


def _run(ev, it=0):
    """one run_evaluation: (TAR, returns, lengths, steps)"""
    tar = ev.run_evaluation(it)
    return tar, ev.returns.copy(), ev.lengths.copy(), ev.steps


def _same(x, y, what):
    assert np.array_equal(_bits(np.array([x[0]])), _bits(np.array([y[0]]))), what      # the TAR's bits
    assert np.array_equal(_bits(x[1]), _bits(y[1])), what
    assert np.array_equal(x[2], y[2]) and x[3] == y[3], what


@pytest.fixture(scope="module")
def shared():
    """one engine for the cases that never write its weights"""
    alg, _ = make_pair(O, A, HID, 64, seed=4)
    return alg


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
NEED = {(5, 7): 13, (33, 40): 13, (5, 70): 96, (5, 3): 8, (1030, 1035): 13}     # lockstep steps an evaluation needs (episode_plan)
CASES = [(n, e, p) for (n, e) in ((5, 7), (33, 40), (5, 70), (5, 3)) for p in (1, 7, 16)] + [(1030, 1035, 7)]


@pytest.mark.parametrize("N,E,P", CASES)
def test_whole_evaluator_equals_the_eager_evaluator(shared, N, E, P):
    from synth_tensor_episodes import episode_plan

    alg = shared
    e = alg.engine
    plans = [episode_plan(k % N, k // N) for k in range(E)]
    busiest = max(sum(episode_plan(r, k)[0] for k in range(len(range(r, E, N)))) for r in range(min(N, E)))
    assert busiest == NEED[(N, E)]
    windows = -(-busiest // P)                                          # per run
    assert 3 * windows - 1 >= 2                                         # three runs always reach the replay stage
    eager, graph = _evaluator(alg, N, E, False, hip_eval_poll_steps=P), _evaluator(alg, N, E, True, hip_eval_poll_steps=P)
    assert graph.graph_eval and not eager.graph_eval
    mode0 = commits0 = None
    for run in range(3):
        want = _run(eager, run)
        polls, mode_calls, commits = (e.debug_get(k) for k in ("eval_polls", "act_mode_dev_calls", "eval_commit_calls"))
        got = _run(graph, run)
        _same(got, want, (run, "graph vs eager"))
        assert got[3] == windows * P
        assert e.debug_get("eval_polls") - polls == windows             # a poll behind every window, outside the graph
        if run == 0:
            mode0, commits0 = e.debug_get("act_mode_dev_calls") - mode_calls, e.debug_get("eval_commit_calls") - commits
    assert [int(n) for n in want[2]] == [p[0] for p in plans]
    kinds = {(te, tr) for _, te, tr in plans}
    if (N, E) in ((33, 40), (5, 70)):                                   # the episode kinds the eager evaluator's own test asserts
        assert (True, False) in kinds and (False, True) in kinds and (True, True) in kinds and 1 in want[2]
    assert graph.graph_captures == 1, "the evaluator never captured"
    assert graph.graph_replays == 3 * windows - 1 >= 2
    assert eager.graph_captures == 0 and eager.graph_replays == 0
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0
    # the counters count HOST calls: the eager window and the capture issued all the graph route ever made
    chunks = (N + 1023) // 1024
    assert chunks == (2 if N == 1030 else 1)
    if windows >= 2:                                                    # (the first run held the eager window and the capture)
        assert mode0 == 2 * P * chunks and commits0 == 2 * P
    else:
        assert mode0 == P * chunks and commits0 == P
    # the actions reach the returns: every one is below the sum of its reward-table entries by the |a|^2 terms
    table = [sum(((37 * (k % N) + 101 * t + 11) % 64) / 16 - 2 for t in range(1, plans[k][0] + 1)) for k in range(E)]
    assert np.isfinite(want[1]).all() and (want[1] < np.array(table) - 1e-3).all()


def test_the_staging_copies_are_off_the_chain(shared, monkeypatch):
    """on the kwarg's route the commit is handed the environment's own tensors and only a window's first acting call reads the
    evaluator's observation buffer -- in the eager window and in the capture (what the replays then repeat)"""
    alg = shared
    e = alg.engine
    N, E, P = 33, 40, 7
    ev = _evaluator(alg, N, E, True, hip_eval_poll_steps=P)
    seen = []
    act_mode_device, eval_commit = e.act_mode_device, e.eval_commit
    monkeypatch.setattr(e, "act_mode_device", lambda obs, act: (seen.append(("act", obs.data_ptr())), act_mode_device(obs, act))[1])
    monkeypatch.setattr(e, "eval_commit", lambda r, te, tr, ended: (seen.append(("commit", r.data_ptr(), te.data_ptr(), tr.data_ptr())),
                                                                   eval_commit(r, te, tr, ended))[1])
    ev.run_evaluation(0)                                                # 13 steps: the eager window and the captured one
    assert ev.graph_captures == 1 and ev.graph_replays == 1
    acts, commits = [c for c in seen if c[0] == "act"], [c for c in seen if c[0] == "commit"]
    assert len(acts) == len(commits) == 2 * P
    own = {ev._rew.data_ptr(), ev._term.data_ptr(), ev._trunc.data_ptr()}
    for i, (a, c) in enumerate(zip(acts, commits)):
        assert (a[1] == ev._obs.data_ptr()) == (i % P == 0), i
        assert not own & set(c[1:]), i


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def test_a_replay_reads_the_live_weights():
    alg, _ = make_pair(O, A, HID, 64, seed=4)
    e = alg.engine
    N, E, P = 33, 40, 7
    ev = _evaluator(alg, N, E, True, hip_eval_poll_steps=P)
    first = _run(ev)
    _same(first, _run(_evaluator(alg, N, E, False, hip_eval_poll_steps=P)), "before")
    assert ev.graph_captures == 1 and ev.graph_replays == 1
    # an update through the library
    rng = np.random.default_rng(0)
    torch.manual_seed(100)
    alg.local_update(synth_batch(rng, 64, O, A), 0)
    after_update = _run(ev, 1)
    _same(after_update, _run(_evaluator(alg, N, E, False, hip_eval_poll_steps=P)), "after local_update")
    # a torch write on the arena, in stream order, and the note that tells the engine
    with torch.cuda.stream(e.torch_stream), torch.no_grad():
        for p in alg.networks.policy.parameters():
            p.mul_(1.25)
    e.note_torch_writes(alg.networks.policy.parameters())
    after_write = _run(ev, 2)
    _same(after_write, _run(_evaluator(alg, N, E, False, hip_eval_poll_steps=P)), "after the torch write")
    assert ev.graph_captures == 1 and ev.graph_replays == 5             # nothing was issued anew: replays only
    assert not np.array_equal(_bits(after_write[1]), _bits(after_update[1]))   # the weights did move the returns
    assert np.array_equal(after_write[2], first[2])                     # ... and never the fixture's episode ends


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_max_steps_off_the_window_grid(shared):
    alg = shared
    e = alg.engine
    N, E, P = 5, 70, 4
    want = _run(_evaluator(alg, N, E, False, hip_eval_poll_steps=P))
    ev = _evaluator(alg, N, E, True, hip_eval_poll_steps=P, hip_eval_max_steps=6)
    polls = e.debug_get("eval_polls")
    with pytest.raises(RuntimeError, match="hip_eval_max_steps = 6"):
        ev.run_evaluation(0)                                            # one (eager, first) window and a 2-step eager remainder
    assert ev.steps == 6 and ev.graph_captures == 0 and ev.graph_replays == 0 and e.debug_get("eval_polls") - polls == 2
    ev.max_steps = 100000
    _same(_run(ev), want, "the full run")                               # (captures on its way)
    assert ev.graph_captures == 1 and ev.graph_replays == 96 // P        # (window 0 ran eagerly in the refused run)
    ev.max_steps = 6
    polls = e.debug_get("eval_polls")
    with pytest.raises(RuntimeError, match="hip_eval_max_steps = 6"):
        ev.run_evaluation(1)                                            # one replayed window and a 2-step eager remainder
    assert ev.steps == 6 and ev.graph_captures == 1 and ev.graph_replays == 96 // P + 1 and e.debug_get("eval_polls") - polls == 2
    # the handle is idle and usable: an eager evaluation with the default limit
    _same(_run(_evaluator(alg, N, E, False, hip_eval_poll_steps=P)), want, "eager after the error")
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_a_reallocation_of_the_bookkeeping_drops_the_graph():
    alg, _ = make_pair(O, A, HID, 64, seed=4)                           # a fresh handle: the state arrays grow from nothing
    e = alg.engine
    N, E, P = 5, 7, 7
    want = _run(_evaluator(alg, N, E, False, hip_eval_poll_steps=P))
    ev = _evaluator(alg, N, E, True, hip_eval_poll_steps=P)
    _same(_run(ev), want, "first")
    assert ev.graph_captures == 1 and ev.graph_replays == 1
    gen = e.debug_get("eval_state_gen")
    assert gen >= 1
    _same(_run(ev), want, "second")
    assert e.debug_get("eval_state_gen") == gen and ev.graph_captures == 1 and ev.graph_replays == 3
    other = _evaluator(alg, N, 70, False)                               # a larger E on the same engine: free + allocate
    other.run_evaluation(0)
    assert e.debug_get("eval_state_gen") == gen + 1
    _same(_run(ev), want, "after the reallocation")                     # eager window, then a new capture
    assert ev.graph_captures == 2 and ev.graph_replays == 4
    _same(_run(ev), want, "replays of the new graph")
    assert ev.graph_captures == 2 and ev.graph_replays == 6
    other.run_evaluation(1)                                             # the same sizes again: nothing moves
    assert e.debug_get("eval_state_gen") == gen + 1
    _same(_run(ev), want, "no reallocation")
    assert ev.graph_captures == 2 and ev.graph_replays == 8


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def _refusals_under_capture(e, calls):
    g = torch.cuda.CUDAGraph()
    from dsact._ffi import DsactError

    refused = []
    with torch.cuda.graph(g, stream=e.torch_stream, capture_error_mode="relaxed"):
        for call in calls:
            try:
                call()
                refused.append(None)
            except DsactError as ex:
                refused.append(str(ex))
    del g
    return refused


def test_library_rules_under_capture():
    alg, _ = make_pair(O, A, HID, 64, seed=4)                           # a fresh handle: it has never acted
    e = alg.engine
    n = 8
    obs, act = torch.zeros(n, O, device="cuda"), torch.full((n, A), float("nan"), device="cuda")
    rew = torch.full((n,), 1.5, device="cuda")
    yes, no = torch.ones(n, dtype=torch.bool, device="cuda"), torch.zeros(n, dtype=torch.bool, device="cuda")
    ended = torch.zeros(n, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    e.eval_begin(n, 2 * n)
    refused = _refusals_under_capture(e, [lambda: e.eval_begin(n, 2 * n), e.eval_poll, lambda: e.eval_read(2 * n),
                                          lambda: e.act_mode_device(obs, act)])
    assert all(r is not None and "E_STATE" in r and "capture" in r for r in refused), refused
    assert "make one call outside the capture first" in refused[3]
    # each refusal left the handle usable and the capture cleanly ended: the eager calls, then a capture of the two legal ones
    e.act_mode_device(obs, act)
    e.eval_commit(rew, yes, no, ended)
    assert e.eval_poll() == n and bool(ended.all())
    want = act.clone()
    assert torch.isfinite(want).all()
    act.fill_(float("nan"))
    ended.zero_()
    mode_calls, commits = e.debug_get("act_mode_dev_calls"), e.debug_get("eval_commit_calls")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=e.torch_stream, capture_error_mode="relaxed"):
        e.act_mode_device(obs, act)
        e.eval_commit(rew, no, yes, ended)
    assert e.debug_get("act_mode_dev_calls") - mode_calls == 1 and e.debug_get("eval_commit_calls") - commits == 1
    e.sync()
    assert bool(torch.isnan(act).all()) and not bool(ended.any()) and e.eval_poll() == n      # captured, not run
    with torch.cuda.stream(e.torch_stream):
        g.replay()
    assert e.eval_poll() == 0 and bool(ended.all())
    assert e.debug_get("act_mode_dev_calls") - mode_calls == 1 and e.debug_get("eval_commit_calls") - commits == 1   # host calls only
    returns, lengths = e.eval_read(2 * n)
    assert returns.tolist() == [1.5] * (2 * n) and lengths.tolist() == [1] * (2 * n)
    assert np.array_equal(_bits(act.cpu().numpy()), _bits(want.cpu().numpy()))
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0
    del g


def test_a_cnn_handle_is_refused_under_capture():
    from dsac_v2_hip import DSAC_V2_HIP
    from test_hip_cnn_parity import cnn_kwargs

    shape, a, n = (3, 96, 96), 3, 4
    torch.manual_seed(3)
    alg = DSAC_V2_HIP(**cnn_kwargs(shape, a, "type_2", 16, hip_cnn_act=True, strict_rng=False))
    e = alg.engine
    assert e.cnn_act
    g = torch.Generator().manual_seed(1)
    frames, act = torch.rand((n,) + shape, generator=g).cuda(), torch.full((n, a), float("nan"), device="cuda")
    torch.cuda.synchronize()
    e.act_mode_device(frames, act)                                      # outside a capture the route serves the handle
    e.sync()
    want = act.clone()
    assert torch.isfinite(want).all()
    refused = _refusals_under_capture(e, [lambda: e.act_mode_device(frames, act)])
    assert all(r is not None and "E_INVALID" in r for r in refused), refused
    assert "under stream capture" in refused[0]
    act.fill_(float("nan"))
    e.act_mode_device(frames, act)                                      # ... and still does
    e.sync()
    assert np.array_equal(_bits(act.cpu().numpy()), _bits(want.cpu().numpy()))


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_training_state_is_untouched():
    import plugin
    from synth_tensor_episodes import SynthTensorEpisodes

    kw = hip_kwargs(O, A, HID, 64, buffer_max_size=400, seed=5, sample_batch_size=64, strict_rng=False)
    torch.manual_seed(1)
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    smp = plugin.create_sampler(**dict(kw, sampler_name="hip_tensor_env_sampler", env=SynthTensorEpisodes(32, device="cuda"),
                                       networks=alg.networks))
    e = alg.engine
    for _ in range(3):
        buf.add_batch(smp.sample()[0])                                  # a ring with 192 rows in it
    arenas = lambda: [t.clone() for t in (e.online, e.target, e.adam_m, e.adam_v)]
    e.sync()
    torch.cuda.synchronize()
    before, state, digest = arenas(), e.get_state(), e.buffer_digest()
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state())
    ev = _evaluator(alg, 33, 40, True)
    for it in range(3):
        assert np.isfinite(ev.run_evaluation(it))
    assert ev.graph_captures == 1 and ev.graph_replays == 2
    e.sync()
    for x, y in zip(before, arenas()):
        assert torch.equal(x, y)
    assert e.get_state() == state and e.buffer_digest() == digest and any(digest)
    assert torch.equal(rng[0], torch.get_rng_state()) and torch.equal(rng[1], torch.cuda.get_rng_state())
    now = np.random.get_state()
    assert rng[2][0] == now[0] and np.array_equal(rng[2][1], now[1]) and rng[2][2:] == now[2:]


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_serial_trainer_ends_bitwise_equal_with_both_graphs(tmp_path):
    import plugin
    from synth_tensor_episodes import SynthTensorEpisodes
    from synth_tensor_episodes_inplace import SynthTensorEpisodesInplace
    from training.hip_trainer import TB, HipOffSerialTrainer, read_scalars

    N, S, iters, cap, warm, every = 32, 64, 120, 4000, 128, 40
    finals, tars = [], []
    for graph in (False, True):
        folder = str(tmp_path / ("graph" if graph else "eager"))
        kw = hip_kwargs(O, A, HID, 64, buffer_max_size=cap, buffer_warm_size=warm, seed=3, sample_batch_size=S,
                        sample_interval=1, max_iteration=iters, log_save_interval=40, apprfunc_save_interval=100000,
                        eval_interval=every, save_folder=folder, ini_network_dir=None, strict_rng=False, hip_device_indices=True,
                        sampler_name="hip_tensor_env_sampler", evaluator_name=NAME, num_eval_episode=40)
        torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
        env = SynthTensorEpisodesInplace if graph else SynthTensorEpisodes
        alg = plugin.create_alg(**kw)
        buf = plugin.create_buffer(**kw)
        smp = plugin.create_sampler(env=env(N, device="cuda"), **dict(kw, **(dict(hip_graph_sample=True) if graph else {})))
        ev = plugin.create_evaluator(eval_env=env(33, device="cuda"), **dict(kw, **(dict(hip_graph_eval=True) if graph else {})))
        assert ev.graph_eval == graph and smp.graph_sample == graph
        tr = plugin.create_trainer(alg, smp, buf, ev, **kw)
        assert type(tr) is HipOffSerialTrainer
        tr.train()
        e = alg.engine
        e.sync()
        assert e.debug_get("handoff_failures") == 0.0 and e.debug_get("act_dev_syncs") == 0.0
        logged = read_scalars(folder)[TB["tar_iter"]]
        assert len(logged["y"]) == 3                                    # evaluations at iterations 0, 40 and 80: one window each
        if graph:
            assert ev.graph_captures == 1 and ev.graph_replays == 2     # eager window, capture (+ its replay), one replay
            assert smp.graph_captures == 1 and smp.graph_replays >= 2
        tars.append([float(y) for y in logged["y"]])
        finals.append((e.buffer_digest(), buf.size, buf.ptr, e.online.cpu().clone(), e.target.cpu().clone(), e.adam_m.cpu().clone(),
                       e.adam_v.cpu().clone()))
    assert np.array_equal(_bits(np.array(tars[0])), _bits(np.array(tars[1]))) and len(set(tars[0])) > 1
    assert finals[0][:3] == finals[1][:3]
    for x, y in zip(finals[0][3:], finals[1][3:]):
        assert torch.equal(x, y)
