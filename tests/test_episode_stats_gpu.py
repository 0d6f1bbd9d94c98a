"""Episode statistics of the training environments on the GPU (k_track_commit / k_track_init, dsact_track_begin /
dsact_track_commit / dsact_track_read, training/hip_tensor_sampler.py with hip_episode_stats):

  1. the kernel alone, driven with scripted rewards and flags: after every commit the whole state equals the NumPy state machine
     of tests/test_episode_stats_host.py (TrackBook) bit for bit, and at the end the per-environment yardstick (reference_state);
     clearing and non-clearing reads; T commits of one step equal one commit of T steps;
  2. through the sampler with a real attached policy on tests/envs/synth_tensor_episodes.py, against the yardstick fed the
     sampler's own DeviceSampleBatch rows;
  3. HipOffSerialTrainer with the statistics on ends bitwise where it ends without them; two runs give the same statistics;
  4. refusals on the real engine leave the handle usable; a larger track_begin after commits starts from clean state.
Every comparison is on fp64 bit patterns and exact integers: nothing needs a tolerance.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs
from test_episode_stats_host import COLUMNS, TrackBook, assert_same_state, bits, reference_state, scripted
from test_hip_parity import make_pair

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

O, A, HID = 17, 6, (64, 64)


@pytest.fixture(scope="module")
def small_engine():
    alg, _ = make_pair(O, A, HID, 64, seed=4)
    return alg


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 5, 33, 300])    # one thread, a partial wave, two workgroups with a ragged tail
def test_kernel_equals_the_restatement_after_every_commit(small_engine, N, T):
    e = small_engine.engine
    commits, clear_at = 7, 3
    rew, term, trunc = scripted(commits * T, N, 1000 * N + T)
    flat = lambda x, c: x[c * T:(c + 1) * T].reshape(-1)
    d_rew, d_term, d_trunc = rew.cuda(), term.cuda(), trunc.cuda()
    torch.cuda.synchronize()                         # the inputs were produced on torch's stream; the calls run on the engine's
    e.track_begin(N)
    book = TrackBook(N)
    calls, reads, syncs = e.debug_get("track_commit_calls"), e.debug_get("track_reads"), e.debug_get("act_dev_syncs")
    assert_same_state(e.track_read(False), book.read(False), "begin")
    for c in range(commits):
        e.track_commit(flat(d_rew, c), flat(d_term, c), flat(d_trunc, c), T)
        book.commit(flat(rew, c).numpy(), flat(term, c).numpy(), flat(trunc, c).numpy(), T)
        want = book.read(False)
        assert_same_state(e.track_read(False), want, c)
        assert_same_state(e.track_read(False), want, (c, "a non-clearing read changes nothing"))
        if c == clear_at:
            assert_same_state(e.track_read(True), book.read(True), (c, "the clearing read returns what was there"))
            after = e.track_read(False)
            assert_same_state(after, book.read(False), (c, "cleared"))
            assert not after["episodes"].any() and not after["terminated"].any() and not after["len_sum"].any()
            assert not after["ret_sum"].any() and not after["last_ret"].any() and not after["last_len"].any()
            assert np.isposinf(after["ret_min"]).all() and np.isneginf(after["ret_max"]).all()
            assert np.array_equal(bits(after["cur_ret"]), bits(want["cur_ret"])) and np.array_equal(after["cur_len"], want["cur_len"])
    assert e.debug_get("track_commit_calls") - calls == commits and e.debug_get("act_dev_syncs") == syncs == 0.0
    assert e.debug_get("track_reads") - reads == 1 + 2 * commits + 2
    final = e.track_read(False)
    R, TE, TR = rew.numpy(), term.numpy(), trunc.numpy()
    assert_same_state(final, reference_state(R, TE, TR, (clear_at + 1) * T), "the per-environment computation")
    assert (TE & TR).any() or commits * T < 2
    if N >= 5:
        assert final["cur_len"][2] == commits * T and final["episodes"][2] == 0            # the row that never ends
        assert final["cur_len"][1] == 0 and final["episodes"][1] == (commits - clear_at - 1) * T   # ... that ends at every step
        assert TE[1, 0] and TR[1, 0]                                                        # both flags in one step
    if N >= 33:
        assert (~(TE | TR)[T - 1::T, 3:]).any()      # episodes are in progress at commit boundaries: the carried pair is at work
    # the same steps as commits of ONE step each (and the clearing read at the same place): the identical state
    e.track_begin(N)                                  # (re-initialises everything)
    for t in range(commits * T):
        e.track_commit(d_rew[t], d_term[t], d_trunc[t], 1)
        if t + 1 == (clear_at + 1) * T:
            e.track_read(True)
    assert_same_state(e.track_read(False), final, "one step per commit")
    # ... and with the fp64 accumulation it is not an fp32 sum's value
    if N >= 33:
        acc = np.zeros(N, np.float32)
        for t in range(commits * T):
            acc = np.where(TE[t] | TR[t], np.float32(0), acc + R[t])
        assert (acc.astype(np.float64) != final["cur_ret"]).any()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,mult", [(5, 1), (5, 3), (33, 1), (33, 3)])
def test_sampler_statistics_equal_the_per_environment_computation(small_engine, N, mult):
    import plugin
    from synth_tensor_episodes import SynthTensorEpisodes
    from training.hip_tensor_sampler import aggregate_episode_rows

    alg = small_engine
    e = alg.engine
    S, calls, clear_at = mult * N, 12, 5
    smp = plugin.create_sampler(sampler_name="hip_tensor_env_sampler", env=SynthTensorEpisodes(N, device="cuda"),
                                sample_batch_size=S, networks=alg.networks, seed=3, reward_scale=0.25, hip_episode_stats=True)
    commits, reads = e.debug_get("track_commit_calls"), e.debug_get("track_reads")
    rew, term, trunc = [], [], []
    clear_step = 0
    for c in range(calls):
        batch, tb = smp.sample()
        assert len(tb) == 1
        e.sync()
        rew.append(batch.rew.cpu().numpy().reshape(mult, N))
        term.append(batch.terminated.cpu().numpy().reshape(mult, N))
        trunc.append(batch.truncated.cpu().numpy().reshape(mult, N))
        R, TE, TR = np.concatenate(rew), np.concatenate(term), np.concatenate(trunc)
        want = reference_state(R, TE, TR, clear_step)
        got = smp.episode_statistics(clear=c == clear_at)
        assert_same_state(got["rows"], want, c)
        agg = aggregate_episode_rows(want)
        for k in ("episodes", "terminated_share", "return_mean", "return_min", "return_max", "length_mean"):
            assert got[k] == agg[k] or (got[k] != got[k] and agg[k] != agg[k]), (c, k)
        if c == clear_at:
            clear_step = len(R)
    assert e.debug_get("track_commit_calls") - commits == calls and e.debug_get("track_reads") - reads == calls
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0
    whole = reference_state(R, TE, TR)
    assert (TE & ~TR).any() and (TR & ~TE).any() and whole["episodes"].min() >= 1 and whole["episodes"].max() >= 4 * mult
    assert mult == 1 or (TE & TR).any()
    # the rewards are the environment's own (reward_scale = 0.25 is the ring's business) and the actions reached them
    assert np.isfinite(whole["ret_sum"]).all() and len(np.unique(R)) > N


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def _train(folder, **stats):
    import plugin
    from synth_tensor_humanoid import SynthTensorHumanoid
    from training.hip_trainer import HipOffSerialTrainer

    o, a, hid, B, N, S, iters, cap, warm = 376, 17, (64, 64), 64, 16, 32, 200, 3000, 64
    kw = hip_kwargs(o, a, hid, B, buffer_max_size=cap, buffer_warm_size=warm, seed=3, sample_batch_size=S, sample_interval=1,
                    max_iteration=iters, log_save_interval=40, apprfunc_save_interval=100000, eval_interval=100000,
                    save_folder=folder, ini_network_dir=None, strict_rng=False, hip_device_indices=True, reward_scale=0.25,
                    sampler_name="hip_tensor_env_sampler", **stats)
    torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    limit = torch.tensor([7, 13, 1000, 29] * (N // 4))
    smp = plugin.create_sampler(env=SynthTensorHumanoid(N, device="cuda", seed=4, episode_limit=limit), **kw)
    tr = plugin.create_trainer(alg, smp, buf, None, **kw)
    assert type(tr) is HipOffSerialTrainer
    tr.train()
    e = alg.engine
    e.sync()
    n_calls = warm // S + iters
    assert smp.get_total_sample_number() == n_calls * S
    out = {"arenas": [t.cpu().clone() for t in (e.online, e.target, e.adam_m, e.adam_v)], "state": e.get_state(),
           "ptr_size": (buf.ptr, buf.size), "act_step": smp.act_step, "index_iteration": buf.index_iteration}
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0
    assert e.debug_get("track_commit_calls") == (n_calls if stats else 0) and e.debug_get("track_reads") == 0.0
    if stats:
        out["stats"] = smp.episode_statistics(clear=False)
        assert e.debug_get("track_reads") == 1.0
        again = smp.episode_statistics(clear=True)
        assert_same_state(again["rows"], out["stats"]["rows"], "a non-clearing read changes nothing")
        assert smp.episode_statistics()["episodes"] == 0 and e.debug_get("track_reads") == 3.0
        assert e.debug_get("act_dev_syncs") == 0.0
    ring = []
    for r0 in range(0, buf.size - B + 1, B):
        e.gather(np.arange(r0, r0 + B))
        got = e.read_batch(with_logp=True)
        ring.append(np.concatenate([np.asarray(got[k]).reshape(B, -1) for k in ("obs", "act", "rew", "obs2", "done", "logp")], axis=1))
    out["ring"] = np.concatenate(ring).view(np.uint32)
    return out, n_calls * S // N


def test_statistics_do_not_perturb_a_training_run(tmp_path):
    off, steps = _train(str(tmp_path / "off"))
    on, _ = _train(str(tmp_path / "on"), hip_episode_stats=True, hip_episode_stats_every=0)
    on2, _ = _train(str(tmp_path / "on2"), hip_episode_stats=True, hip_episode_stats_every=0)
    for other in (on, on2):
        for x, y in zip(off["arenas"], other["arenas"]):
            assert torch.equal(x, y)
        assert np.array_equal(off["ring"], other["ring"]) and off["ring"].shape[0] >= 3000 // 64 * 64
        for k in ("state", "ptr_size", "act_step", "index_iteration"):
            assert off[k] == other[k], k
    assert off["act_step"] == steps and "stats" not in off
    a, b = on["stats"], on2["stats"]
    assert_same_state(a["rows"], b["rows"], "two runs")
    for k in ("episodes", "terminated_share", "return_mean", "return_min", "return_max", "length_mean"):
        assert a[k] == b[k], k
    rows = a["rows"]
    # every lockstep step is in exactly one place: a finished episode or the one in progress
    assert np.array_equal(rows["len_sum"] + rows["cur_len"], np.full(16, steps))
    # limits 7, 13, 1000, 29 by row: the time-outs and the early terminations are both there
    assert a["episodes"] >= 16 // 4 * (steps // 7) and 0.0 < a["terminated_share"] < 1.0
    assert (rows["len_sum"][0::4] // rows["episodes"][0::4] <= 7).all() and a["return_min"] <= a["return_mean"] <= a["return_max"]


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from dsact._ffi import DsactError

    alg, _ = make_pair(O, A, HID, 64, seed=4)       # a fresh handle: no dsact_track_begin yet
    e = alg.engine
    n = 8
    rew = torch.full((n,), 1.5, device="cuda")
    off, on = torch.zeros(n, dtype=torch.bool, device="cuda"), torch.ones(n, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(DsactError, match="E_STATE.*before dsact_track_begin"):
        e.track_commit(rew, off, off, 1)
    with pytest.raises(DsactError, match="E_STATE.*before dsact_track_begin"):
        e.track_read()
    with pytest.raises(DsactError, match="E_INVALID"):
        e.track_begin(0)
    e.track_begin(n)
    with pytest.raises(DsactError, match="E_INVALID.*n_steps"):
        e.track_commit(rew, off, off, 0)
    # host pointers (pageable and pinned) and a wrong n_envs at the C-ABI itself: the Python wrapper would refuse them first
    lib, h = e._lib, e._h
    P = lambda t: C.c_void_p(t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr())
    h_rew, h_flag = np.zeros(n, np.float32), np.zeros(n, np.uint8)
    p_rew, p_flag = torch.zeros(n).pin_memory(), torch.zeros(n, dtype=torch.uint8).pin_memory()
    for args in ((h_rew, off, off), (rew, h_flag, off), (rew, off, h_flag), (p_rew, off, off), (rew, p_flag, off), (rew, off, p_flag)):
        assert lib.dsact_track_commit(h, *[P(x) for x in args], 1) == -1
        assert b"device pointers" in lib.dsact_last_error(h)
    host = {k: np.zeros(n + 1, dt) for k, dt in COLUMNS}
    for wrong in (n - 1, n + 1, 0):
        assert lib.dsact_track_read(h, wrong, *[P(a) for a in host.values()], 1) == -1
        assert b"n_envs" in lib.dsact_last_error(h)
    assert e.debug_get("track_commit_calls") == 0.0 and e.debug_get("track_reads") == 0.0
    with pytest.raises(ValueError, match="reward must be a torch tensor on"):
        e.track_commit(torch.zeros(n), off, off, 1)
    with pytest.raises(ValueError, match="dtype"):
        e.track_commit(rew.double(), off, off, 1)
    with pytest.raises(ValueError, match="shape"):
        e.track_commit(rew, off, off, 2)
    # ... and the handle works: nothing above reached the state
    assert_same_state(e.track_read(False), TrackBook(n).read(False))
    e.track_commit(rew, off, off, 1)
    e.track_commit(rew, on, off, 1)
    got = e.track_read(False)
    assert got["episodes"].tolist() == [1] * n and got["terminated"].tolist() == [1] * n and got["ret_sum"].tolist() == [3.0] * n
    assert got["last_len"].tolist() == [2] * n and got["cur_len"].tolist() == [0] * n
    e.track_commit(rew, off, off, 1)                 # an episode in progress ...
    # ... and a track_begin with a larger N (a new block) starts from clean state
    big = 700
    e.track_begin(big)
    assert_same_state(e.track_read(False), TrackBook(big).read(False), "a larger begin")
    r2 = torch.full((big,), 0.25, device="cuda")
    f2 = torch.zeros(big, dtype=torch.bool, device="cuda")
    t2 = ~f2
    torch.cuda.synchronize()
    e.track_commit(r2, f2, t2, 1)
    got = e.track_read()
    assert got["episodes"].tolist() == [1] * big and got["terminated"].tolist() == [0] * big and got["ret_min"].tolist() == [0.25] * big
    e.track_begin(n)                                 # a smaller one reuses the block, and is clean as well
    assert_same_state(e.track_read(False), TrackBook(n).read(False), "a smaller begin")
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0
    assert np.isfinite(e.act_mode_batch(torch.zeros(4, O, device="cuda"))).all()
