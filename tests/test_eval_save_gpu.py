"""eval_save on the device-resident evaluator, on the GPU (k_eval_record, k_eval_commit<true>, dsact_eval_trace_* /
dsact_eval_record, training/hip_tensor_evaluator.py with eval_save=True). Everything is compared BITWISE:
the feature is a copy.

  1. k_eval_record + k_eval_commit<true> alone, driven with scripted observations, actions, rewards and flags, against the NumPy
     restatement of tests/test_eval_save_host.py: every stored slot, rows per episode, the dropped counter, the fill in the slots
     nothing may write, and the bookkeeping against the run without a trace;
  2. image rows (byte and fp32 frames) on a handle with the CNN acting path;
  3. the whole evaluator on tests/envs/synth_tensor_episodes.py against a restatement (act_mode_batch per step + the NumPy trace);
  4. the graph route: files bitwise the eager route's, one capture, and the generation guard over the trace's arrays;
  5. slot offsets past 2^31 bytes;
  6. library refusals that leave the handle usable;
  7. HipOffSerialTrainer with eval_save ends bitwise where the run without it ends, and writes the same files twice.
"""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from helpers import hip_kwargs
from test_eval_save_host import FILL, TraceEngine, closed_form_episode, files_of, load, same
from test_hip_parity import make_pair

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

HID, M = (64, 64), 4
NAME = "hip_tensor_env_evaluator"
_engines = {}


def _alg(O, A):
    if (O, A) not in _engines:
        _engines[(O, A)] = make_pair(O, A, HID, 64, seed=4)[0]
    return _engines[(O, A)]


def _quiet(e):
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def _script(N, E, O, A, seed):
    """a scripted evaluation: episode j of row i lasts 1 + (7 i + 3 j + 3) % 11 steps (1 .. 11) and ends terminated, truncated or
    both by (i + j) % 3; observations are arbitrary bit patterns (NaNs included), actions and rewards finite floats"""
    g = torch.Generator().manual_seed(seed)
    lens = [[1 + (7 * i + 3 * j + 3) % 11 for j in range(len(range(i, E, N)))] for i in range(N)]
    T = max(sum(l) for l in lens) + 1                       # one more: commits past the end count nothing
    term, trunc = torch.rand(T, N, generator=g) < 0.3, torch.rand(T, N, generator=g) < 0.3   # (rows without an episode: anything)
    for i in range(N):
        t = 0
        for j, n in enumerate(lens[i]):
            term[t:t + n, i] = trunc[t:t + n, i] = False
            term[t + n - 1, i], trunc[t + n - 1, i] = (i + j) % 3 != 1, (i + j) % 3 != 0
            t += n
    obs = torch.randint(-2 ** 31, 2 ** 31 - 1, (T, N, O), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32).contiguous()
    act = torch.randn(T, N, A, generator=g).contiguous()
    rew = (torch.randn(T, N, generator=g) * torch.tensor(10.0) ** torch.randint(-3, 4, (T, N), generator=g).float()).contiguous()
    return dict(T=T, lens=lens, obs=obs, act=act, rew=rew, term=term, trunc=trunc)


def _uniform(N, E, O, A, value):
    """every episode lasts exactly M steps: rounds of M steps whose last one ends every row; all rows hold `value` bytes"""
    T = -(-E // N) * M
    end = torch.zeros(T, N, dtype=torch.bool)
    end[M - 1::M] = True
    byte = torch.full((T, N, 4 * O), value, dtype=torch.uint8).view(torch.float32).contiguous()
    return dict(T=T, obs=byte, act=torch.full((T, N, A), 0.25 + value), rew=torch.full((T, N), 0.5 + value), term=end, trunc=torch.zeros_like(end))


def _drive(e, s, N, E, n_saved, record, poll=False):
    """one scripted evaluation on the real engine: (returns, lengths, ended[T, N], remaining per step)"""
    d = {k: s[k].cuda() for k in ("obs", "act", "rew", "term", "trunc")}
    ended = torch.zeros(s["T"], N, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    e.eval_begin(N, E)
    if n_saved:
        e.eval_trace_begin(n_saved, M, 4 * e.obs_dim)
    left = []
    for t in range(s["T"]):
        if record:
            e.eval_record(d["obs"][t], d["act"][t])
        e.eval_commit(d["rew"][t], d["term"][t], d["trunc"][t], ended[t])
        if poll:
            left.append(e.eval_poll())
    assert e.eval_poll() == 0
    returns, lengths = e.eval_read(E)
    return returns, lengths, ended.cpu(), left


@pytest.mark.parametrize("N", [5, 33, 300])
@pytest.mark.parametrize("O,A", [(3, 1), (3, 6), (16, 1), (16, 6), (17, 1), (17, 6)])
def test_record_and_traced_commit_equal_the_restatement(O, A, N):
    e = _alg(O, A).engine
    for E in (3, N, 4 * N + 1):
        s = _script(N, E, O, A, 1000 * N + E)
        plain = _drive(e, s, N, E, 0, False, poll=True)                 # the run with no trace
        assert max(max(l) for l in s["lens"] if l) > M >= min(min(l) for l in s["lens"] if l)     # episodes past the trace's end and inside it
        for n_saved in sorted({1, E - 1, E}):
            # a. the fill: an evaluation that writes FILL bytes into every slot of the first n_saved episodes
            _drive(e, _uniform(N, E, O, A, FILL), N, E, n_saved, True)
            e.eval_trace_end()
            # b. the scripted evaluation, on the engine and on the restatement
            records, commits, syncs = e.debug_get("eval_record_calls"), e.debug_get("eval_commit_calls"), e.debug_get("act_dev_syncs")
            got = _drive(e, s, N, E, n_saved, True, poll=True)
            assert e.debug_get("eval_record_calls") - records == e.debug_get("eval_commit_calls") - commits == s["T"]
            assert e.debug_get("act_dev_syncs") == syncs
            ref = TraceEngine(O, A)
            ref.eval_begin(N, E)
            ref.eval_trace_begin(n_saved, M, 4 * O)
            ended_ref = torch.zeros(s["T"], N, dtype=torch.bool)
            for t in range(s["T"]):
                ref.eval_record(s["obs"][t], s["act"][t])
                ref.eval_commit(s["rew"][t], s["term"][t], s["trunc"][t], ended_ref[t])
            assert ref.remaining == 0
            # the bookkeeping is the run without a trace, and the restatement's
            for x, y in zip(got, plain):
                assert same(x, y) if isinstance(x, np.ndarray) else (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y)
            assert same(got[0], ref.returns) and same(got[1], ref.lengths) and torch.equal(got[2], ended_ref)
            want_dropped = sum(max(0, n - M) for i in range(N) for j, n in enumerate(s["lens"][i]) if i + j * N < n_saved)
            assert e.debug_get("eval_trace_dropped") == want_dropped == ref.dropped and (n_saved < 3 or want_dropped > 0)
            rows = []
            for ep in range(n_saved):
                n = min(int(got[1][ep]), M)
                assert int(got[1][ep]) == s["lens"][ep % N][ep // N]
                obs, act, rew = e.eval_trace_read(ep, n)
                assert obs.shape == (n, 4 * O) and act.shape == (n, A) and rew.shape == (n,)
                assert same(obs, ref.tr_obs[ep, :n]) and same(act, ref.tr_act[ep, :n]) and same(rew, ref.tr_rew[ep, :n]), (N, E, n_saved, ep)
                rows.append(n)
            e.eval_trace_end()
            # c. the slots nothing may have written still hold the fill: an evaluation of M-step episodes WITHOUT records reads
            # all M slots of every saved episode back (its commits store the rewards only)
            u = _uniform(N, E, O, A, 0)
            _drive(e, u, N, E, n_saved, False)
            for ep in range(n_saved):
                obs, act, rew = e.eval_trace_read(ep, M)
                n = rows[ep]
                assert obs.shape == (M, 4 * O) and same(obs[:n], ref.tr_obs[ep, :n]) and same(act[:n], ref.tr_act[ep, :n])
                assert (obs[n:] == FILL).all() and (act[n:] == np.float32(0.25 + FILL)).all(), (N, E, n_saved, ep)
                assert (rew == np.float32(0.5)).all()
            e.eval_trace_end()
    _quiet(e)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", ["uint8", "float32"])
def test_image_rows_keep_dtype_shape_and_bits(frames, tmp_path):
    import plugin
    from synth_tensor_blob import SHAPE, SynthTensorBlob
    from test_tensor_image_gpu import BOOK, _make

    N, E = 5, 7
    alg = _make(SHAPE, 3, "type_2", book=BOOK if frames == "uint8" else None)[0]
    e = alg.engine
    env = SynthTensorBlob(N, device="cuda", seed=6, frames=frames)
    seen = []
    reset = env.reset
    env.reset = lambda *a: (seen.append(reset(*a).clone()), seen[-1])[1]      # what the evaluator reads at lockstep step len(seen) - 1
    ev = plugin.create_evaluator(evaluator_name=NAME, eval_env=env, num_eval_episode=E, networks=alg.networks, hip_cnn_act=True,
                                 hip_eval_poll_steps=8, eval_save=True, save_folder=str(tmp_path), hip_eval_save_max_steps=20)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ev.run_evaluation(0)
    assert files_of(tmp_path) == ["iter0_ep%d.npy" % k for k in range(E)] and list(ev.lengths) == [20] * E and ev.trace_dropped == 0
    dtype = np.uint8 if frames == "uint8" else np.float32
    for ep_i in range(E):
        ep = load(tmp_path / "evaluator" / ("iter0_ep%d.npy" % ep_i))
        r, k = ep_i % N, ep_i // N
        want = torch.stack([seen[20 * k + t][r] for t in range(20)]).cpu().numpy()
        assert len(ep["obs_list"]) == 20 and all(o.dtype == dtype and o.shape == SHAPE for o in ep["obs_list"])
        assert same(np.stack(ep["obs_list"]), want), ep_i
        acc = np.float64(0.0)
        for x in ep["reward_list"]:
            assert type(x) is float and float(np.float32(x)) == x
            acc = acc + np.float64(x)
        assert same(acc, ev.returns[ep_i])
        for t in (0, 19):                                   # the action rows: the acting call on the frames of that lockstep step
            out = torch.full((N, 3), float("nan"), device="cuda")
            torch.cuda.synchronize()
            e.act_mode_device(seen[20 * k + t], out)
            e.sync()
            assert same(ep["action_list"][t], out[r].cpu().numpy()), (ep_i, t)
    assert len({o.tobytes() for o in load(tmp_path / "evaluator" / "iter0_ep0.npy")["obs_list"]}) > 1
    _quiet(e)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def _restatement(e, N, E, saved, max_steps):
    """act_mode_batch per lockstep step over all rows, the NumPy trace and bookkeeping, the same environment class; the
    observations are held to the fixture's closed forms below"""
    from synth_tensor_episodes import SynthTensorEpisodes

    env = SynthTensorEpisodes(N, device="cuda")
    book = TraceEngine(e.obs_dim, e.act_dim)
    book.eval_begin(N, E)
    book.eval_trace_begin(saved, max_steps, 4 * e.obs_dim)
    obs = env.reset()
    ended = torch.zeros(N, dtype=torch.bool)
    while book.remaining:
        act = torch.from_numpy(e.act_mode_batch(obs.contiguous()))
        book.eval_record(obs.cpu(), act)
        obs2, rew, term, trunc = env.step(act.cuda())
        book.eval_commit(rew.cpu(), term.cpu(), trunc.cpu(), ended)
        obs = env.reset(ended.cuda())
    return book


def _check_files(folder, iteration, k0, book, saved):
    for ep_i in range(saved):
        ep = load(os.path.join(str(folder), "evaluator", "iter%s_ep%d.npy" % (iteration, k0 + ep_i)))
        n = min(int(book.lengths[ep_i]), book.max_steps)
        assert list(ep) == ["reward_list", "action_list", "obs_list"] and len(ep["reward_list"]) == len(ep["action_list"]) == len(ep["obs_list"]) == n
        assert all(type(x) is float for x in ep["reward_list"]) and all(o.shape == (book.obs_dim,) for o in ep["obs_list"])
        assert same(np.array(ep["reward_list"], np.float64).astype(np.float32), book.tr_rew[ep_i, :n]), ep_i
        assert same(np.stack(ep["action_list"]), book.tr_act[ep_i, :n]), ep_i
        assert same(np.ascontiguousarray(np.stack(ep["obs_list"])).view(np.uint8), book.tr_obs[ep_i, :n]), ep_i
        closed = closed_form_episode(ep_i % book.N, ep_i // book.N, book.max_steps)[0]
        assert same(np.stack(ep["obs_list"]), np.stack(closed)), ep_i


@pytest.mark.parametrize("N,E", [(5, 7), (33, 40)])
def test_whole_evaluator_files_equal_the_restatement(N, E, tmp_path):
    import plugin
    from synth_tensor_episodes import SynthTensorEpisodes

    alg = _alg(17, 6)
    e = alg.engine
    book = _restatement(e, N, E, E, 11)
    arenas = lambda: [t.clone() for t in (e.online, e.target, e.adam_m, e.adam_v)]
    e.sync()
    torch.cuda.synchronize()
    before, state = arenas(), e.get_state()
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state())
    for P in (1, 7, 64):
        make = lambda **over: plugin.create_evaluator(evaluator_name=NAME, eval_env=SynthTensorEpisodes(N, device="cuda"), num_eval_episode=E,
                                                      networks=alg.networks, hip_eval_poll_steps=P, **over)
        plain, folder = make(), tmp_path / ("p%d" % P)
        ev = make(eval_save=True, save_folder=str(folder), hip_eval_save_max_steps=11)
        for again in range(2):
            records = e.debug_get("eval_record_calls")
            want_tar = plain.run_evaluation(again)
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                tar = ev.run_evaluation(again)
            assert same(np.float64(tar), np.float64(want_tar)) and same(ev.returns, plain.returns) and same(ev.lengths, plain.lengths)
            assert same(ev.returns, book.returns) and same(ev.lengths, book.lengths) and ev.steps == plain.steps
            assert e.debug_get("eval_record_calls") - records == ev.steps and ev.trace_dropped == 0
            assert files_of(folder) == sorted("iter%d_ep%d.npy" % (it, k) for it in range(again + 1) for k in range(E))
            _check_files(folder, again, 0, book, E)
    # episodes longer than the trace, and fewer saved episodes than played
    cut = _restatement(e, N, E, 2, M)
    ev = plugin.create_evaluator(evaluator_name=NAME, eval_env=SynthTensorEpisodes(N, device="cuda"), num_eval_episode=E, networks=alg.networks,
                                 hip_eval_poll_steps=7, eval_save=True, save_folder=str(tmp_path / "cut"), hip_eval_save_max_steps=M,
                                 hip_eval_save_episodes=2)
    if cut.dropped:
        with pytest.warns(RuntimeWarning, match="hip_eval_save_max_steps = 4"):
            ev.run_evaluation(0)
    else:
        ev.run_evaluation(0)
    assert ev.trace_dropped == cut.dropped and same(ev.returns, book.returns) and files_of(tmp_path / "cut") == ["iter0_ep0.npy", "iter0_ep1.npy"]
    _check_files(tmp_path / "cut", 0, 0, cut, 2)
    # the training state and the generators are where they were
    e.sync()
    for x, y in zip(before, arenas()):
        assert torch.equal(x, y)
    assert e.get_state() == state
    assert torch.equal(rng[0], torch.get_rng_state()) and torch.equal(rng[1], torch.cuda.get_rng_state())
    now = np.random.get_state()
    assert rng[2][0] == now[0] and np.array_equal(rng[2][1], now[1]) and rng[2][2:] == now[2:]
    _quiet(e)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_graph_route_writes_the_eager_files_and_guards_the_trace_arrays(tmp_path):
    import plugin
    from synth_tensor_episodes import SynthTensorEpisodes
    from synth_tensor_episodes_inplace import SynthTensorEpisodesInplace

    N, E, P = 33, 40, 7
    alg_e, alg_g = make_pair(17, 6, HID, 64, seed=4)[0], make_pair(17, 6, HID, 64, seed=4)[0]
    kw = dict(evaluator_name=NAME, num_eval_episode=E, hip_eval_poll_steps=P, eval_save=True, hip_eval_save_max_steps=11)
    eager = plugin.create_evaluator(eval_env=SynthTensorEpisodes(N, device="cuda"), networks=alg_e.networks, save_folder=str(tmp_path / "eager"), **kw)
    graph = plugin.create_evaluator(eval_env=SynthTensorEpisodesInplace(N, device="cuda"), networks=alg_g.networks, hip_graph_eval=True,
                                    save_folder=str(tmp_path / "graph"), **kw)
    eg = alg_g.engine
    records = eg.debug_get("eval_record_calls")
    for run in range(3):
        tar_e, tar_g = eager.run_evaluation(run), graph.run_evaluation(run)
        assert same(np.float64(tar_e), np.float64(tar_g)) and same(eager.returns, graph.returns) and same(eager.lengths, graph.lengths)
        assert eager.steps == graph.steps
    assert graph.graph_captures == 1 and graph.graph_replays == 3 * (graph.steps // P) - 1
    assert eg.debug_get("eval_record_calls") - records == 2 * P          # host calls: the eager window and the capture hold record nodes
    names = files_of(tmp_path / "eager")
    assert names == files_of(tmp_path / "graph") and len(names) == 3 * E
    for n in names:
        a, b = load(tmp_path / "eager" / "evaluator" / n), load(tmp_path / "graph" / "evaluator" / n)
        assert a["reward_list"] == b["reward_list"] and len(a["reward_list"]) >= 1
        assert same(np.stack(a["action_list"]), np.stack(b["action_list"])) and same(np.stack(a["obs_list"]), np.stack(b["obs_list"])), n
        assert (tmp_path / "eager" / "evaluator" / n).read_bytes() == (tmp_path / "graph" / "evaluator" / n).read_bytes(), n
    # a second evaluator whose dsact_eval_begin reallocates drops the graph through eval_state_gen, as without the kwarg ...
    gen = eg.debug_get("eval_state_gen")
    big = plugin.create_evaluator(evaluator_name=NAME, eval_env=SynthTensorEpisodes(70, device="cuda"), num_eval_episode=75, networks=alg_g.networks)
    big.run_evaluation(0)
    assert eg.debug_get("eval_state_gen") == gen + 1
    graph.run_evaluation(3)
    assert graph.graph_captures == 2 and same(graph.returns, eager.returns)
    # ... and so does one whose trace is larger: the arrays the record nodes hold are gone
    gen = eg.debug_get("eval_state_gen")
    wide = plugin.create_evaluator(eval_env=SynthTensorEpisodes(N, device="cuda"), networks=alg_g.networks, save_folder=str(tmp_path / "wide"),
                                   **dict(kw, hip_eval_save_max_steps=64))
    wide.run_evaluation(0)
    assert eg.debug_get("eval_state_gen") == gen + 1
    graph.run_evaluation(4)
    eager.run_evaluation(4)
    assert graph.graph_captures == 3 and same(graph.returns, eager.returns)
    for k in range(E):
        n = "iter4_ep%d.npy" % k
        assert (tmp_path / "eager" / "evaluator" / n).read_bytes() == (tmp_path / "graph" / "evaluator" / n).read_bytes(), n
    _quiet(eg)
    for alg in (alg_e, alg_g):
        alg.engine.close()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_slot_offsets_past_two_to_the_31_bytes():
    if torch.cuda.mem_get_info()[0] < 8 * 1024 ** 3:
        pytest.skip("less than 8 GB of device memory free")
    O, A, N, S = 17, 1, 3, 16_000_000
    e = make_pair(O, A, HID, 64, seed=4)[0].engine
    try:
        assert 2 * S * 4 * O > 2 ** 31                                   # the last saved episode's observation slots
        g = torch.Generator().manual_seed(5)
        obs, act, rew = torch.randn(2, N, O, generator=g).cuda(), torch.randn(2, N, A, generator=g).cuda(), torch.randn(2, N, generator=g).cuda()
        end = torch.tensor([[False] * N, [True] * N]).cuda()
        none, ended = torch.zeros(N, dtype=torch.bool, device="cuda"), torch.zeros(N, dtype=torch.bool, device="cuda")
        torch.cuda.synchronize()
        e.eval_begin(N, N)
        e.eval_trace_begin(N, S, 4 * O)
        for t in range(2):
            e.eval_record(obs[t], act[t])
            e.eval_commit(rew[t], end[t], none, ended)
        assert e.eval_poll() == 0
        returns, lengths = e.eval_read(N)
        assert list(lengths) == [2] * N
        for ep in range(N):
            o, a, r = e.eval_trace_read(ep, 2)
            assert same(o.view(np.float32), obs[:, ep].cpu().numpy()) and same(a, act[:, ep].cpu().numpy()) and same(r, rew[:, ep].cpu().numpy()), ep
        assert e.debug_get("eval_trace_dropped") == 0.0
        e.eval_trace_end()
        _quiet(e)
    finally:
        e.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_library_refusals_leave_the_handle_usable():
    from dsact._ffi import DsactError

    O, A, n = 17, 6, 8
    e = make_pair(O, A, HID, 64, seed=4)[0].engine      # a fresh handle: no trace yet
    f = lambda *s: torch.zeros(*s, device="cuda")
    obs, act, rew = f(n, O) + 0.25, f(n, A) + 0.5, f(n) + 1.5
    flags, ended = torch.zeros(n, dtype=torch.bool, device="cuda"), torch.zeros(n, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(DsactError, match="E_STATE.*before dsact_eval_begin"):
        e.eval_trace_begin(1, 4, 4 * O)
    e.eval_begin(n, 4)
    with pytest.raises(DsactError, match="E_STATE.*without an active trace"):
        e.eval_record(obs, act)
    for bad in (4 * O + 4, O, 0, 16 * O):
        with pytest.raises(DsactError, match="E_INVALID.*obs_row_bytes"):
            e.eval_trace_begin(1, 4, bad)
    for n_saved, steps in ((0, 4), (5, 4), (1, 0)):
        with pytest.raises(DsactError, match="E_INVALID"):
            e.eval_trace_begin(n_saved, steps, 4 * O)
    with pytest.raises(DsactError, match="E_STATE.*without an active trace"):
        e.eval_record(obs, act)                                          # a refused begin leaves no trace behind
    e.eval_trace_begin(2, 4, 4 * O)
    # host pointers (pageable and pinned) at the C-ABI itself: the Python wrapper would refuse them first
    P = lambda t: C.c_void_p(t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr())
    lib, h = e._lib, e._h
    h_obs, h_act, pinned = np.zeros((n, O), np.float32), np.zeros((n, A), np.float32), torch.zeros(n, O).pin_memory()
    for args in ((h_obs, act), (pinned, act), (obs, h_act)):
        assert lib.dsact_eval_record(h, *[P(x) for x in args]) == -1
        assert b"device pointers" in lib.dsact_last_error(h)
    assert e.debug_get("eval_record_calls") == 0.0
    with pytest.raises(ValueError, match="obs must be a torch tensor on"):
        e.eval_record(torch.zeros(n, O), act)
    with pytest.raises(ValueError, match="shape"):
        e.eval_record(obs, f(n, A + 1))
    # ... while episodes remain; then a capacity that is too small
    e.eval_record(obs, act)
    e.eval_commit(rew, flags, flags, ended)
    with pytest.raises(DsactError, match="E_STATE.*have not ended"):
        e.eval_trace_read(0, 4)
    e.eval_record(obs + 1, act + 1)
    e.eval_commit(rew + 1, ~flags, flags, ended)
    assert e.eval_poll() == 0
    with pytest.raises(DsactError, match="E_INVALID.*capacity_rows"):
        e.eval_trace_read(0, 1)
    with pytest.raises(DsactError, match="E_INVALID.*episode"):
        e.eval_trace_read(2, 4)
    # ... and the handle works
    returns, lengths = e.eval_read(4)
    assert returns.tolist() == [4.0] * 4 and lengths.tolist() == [2] * 4
    for ep in range(2):
        o, a, r = e.eval_trace_read(ep, 2)
        assert o.view(np.float32).tolist() == [[0.25] * O, [1.25] * O] and a.tolist() == [[0.5] * A, [1.5] * A] and r.tolist() == [1.5, 2.5]
    e.eval_trace_end()
    with pytest.raises(DsactError, match="E_STATE.*without an active trace"):
        e.eval_trace_read(0, 2)
    # a new dsact_eval_begin starts without a trace
    e.eval_trace_begin(2, 4, 4 * O)
    e.eval_begin(n, 4)
    with pytest.raises(DsactError, match="E_STATE.*without an active trace"):
        e.eval_record(obs, act)
    _quiet(e)
    e.close()


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_serial_trainer_with_eval_save_ends_where_the_run_without_it_ends(tmp_path):
    import plugin
    from synth_tensor_episodes import SynthTensorEpisodes
    from training.hip_trainer import HipOffSerialTrainer

    O, A, N, S, iters, every = 17, 6, 32, 64, 60, 20
    finals, tars, folders = [], [], []
    for run, save in enumerate((False, True, True)):
        folder = str(tmp_path / ("run%d" % run))
        kw = hip_kwargs(O, A, HID, 64, buffer_max_size=4000, buffer_warm_size=128, seed=3, sample_batch_size=S, sample_interval=1,
                        max_iteration=iters, log_save_interval=40, apprfunc_save_interval=100000, eval_interval=every, save_folder=folder,
                        ini_network_dir=None, strict_rng=False, hip_device_indices=True, sampler_name="hip_tensor_env_sampler",
                        evaluator_name=NAME, num_eval_episode=40, **(dict(eval_save=True, hip_eval_save_max_steps=11) if save else {}))
        torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
        alg = plugin.create_alg(**kw)
        buf = plugin.create_buffer(**kw)
        smp = plugin.create_sampler(env=SynthTensorEpisodes(N, device="cuda"), **kw)
        ev = plugin.create_evaluator(eval_env=SynthTensorEpisodes(33, device="cuda"), **kw)
        assert ev.eval_save is save
        seen = []
        run_evaluation = ev.run_evaluation
        ev.run_evaluation = lambda it: (seen.append((it, run_evaluation(it), ev.returns.copy(), ev.lengths.copy())), seen[-1][1])[1]
        tr = plugin.create_trainer(alg, smp, buf, ev, **kw)
        assert type(tr) is HipOffSerialTrainer
        tr.train()
        e = alg.engine
        e.sync()
        assert [s[0] for s in seen] == list(range(0, iters, every)) and len(seen) == 3
        _quiet(e)
        finals.append([t.cpu().clone() for t in (e.online, e.target, e.adam_m, e.adam_v)])
        tars.append(seen)
        folders.append(folder)
        e.close()
    for other in (1, 2):
        for x, y in zip(finals[0], finals[other]):
            assert torch.equal(x, y)
        for s0, s1 in zip(tars[0], tars[other]):
            assert same(np.float64(s0[1]), np.float64(s1[1])) and same(s0[2], s1[2]) and same(s0[3], s1[3])
    assert files_of(folders[0]) == []
    names = files_of(folders[1])
    assert names == files_of(folders[2]) == sorted("iter%d_ep%d.npy" % (it, k) for it in range(0, iters, every) for k in range(40))
    for n in names:
        assert open(os.path.join(folders[1], "evaluator", n), "rb").read() == open(os.path.join(folders[2], "evaluator", n), "rb").read(), n
    first, last = load(os.path.join(folders[1], "evaluator", "iter0_ep0.npy")), load(os.path.join(folders[1], "evaluator", "iter40_ep0.npy"))
    assert not same(np.stack(first["action_list"]), np.stack(last["action_list"]))          # the policy moved between evaluations
