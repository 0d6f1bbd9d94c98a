"""Device-resident image environments on the GPU: dsact_act_sample_device / dsact_act_mode_device /
dsact_buffer_add_device on a CNN handle with dsact_cnn_acting_enable, from fp32 frames and from byte frames (codes into the coded
ring's codebook: k_act_frames_u8, k_ring_commit_codes), the event that orders a held call behind a device-resident one, and
the sampler / evaluator / serial trainer on tests/envs/synth_tensor_blob.py.

Shapes: (3, 96, 96) type_2 with A = 3 takes the RGB ingest forms, (4, 84, 84) type_1 with A = 2 the generic fp32 form and the
4-channel byte form. Handles are built at batch 16. Every test fails on a tree without the feature: the calls are refused there.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from test_hip_cnn_parity import cnn_kwargs
from test_tensor_sampler_gpu import _HostRing
from test_vec_acting import _check, _cpu_twin, _reference

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

SHAPES = [pytest.param((4, 84, 84), 2, "type_1", id="type_1"), pytest.param((3, 96, 96), 3, "type_2", id="type_2")]
BOOK = np.float32(np.arange(256) / 255.0)
LIM, B = 1.0, 16
_cache = {}


def _kw(shape, A, ct, **over):
    return cnn_kwargs(shape, A, ct, B, hip_cnn_act=True, strict_rng=False, **over)


def _make(shape, A, ct, cap=40, book=None, seed=3, **over):
    """(alg, buffer): an enabled CNN handle with a ring of `cap` rows (book: a coded ring)"""
    from dsac_v2_hip import DSAC_V2_HIP
    from training.hip_replay_buffer import HipReplayBuffer

    torch.manual_seed(seed)
    kw = _kw(shape, A, ct, buffer_max_size=cap, **over)
    alg = DSAC_V2_HIP(**kw)
    buf = HipReplayBuffer(**dict(kw, hip_engine=alg.engine, hip_obs_codebook=book))
    assert buf.engine is alg.engine and alg.engine.cnn_act
    return alg, buf


def _shared(shape, A, ct):
    """(alg with a coded ring, codes[70], frames[70] = BOOK[codes], eps[70], the n = 70 batch call's results): built once per
    shape, never written afterwards"""
    key = (shape, A, ct)
    if key not in _cache:
        alg, _ = _make(shape, A, ct, book=BOOK)
        rng = np.random.default_rng(7)
        codes = rng.integers(0, 256, (70,) + tuple(shape), dtype=np.uint8)
        obs = BOOK[codes]
        eps = rng.standard_normal((70, A)).astype(np.float32)
        a, lp = alg.engine.act_sample_batch(obs, eps)
        _cache[key] = (alg, codes, obs, eps, (a.copy(), lp.copy()))
    return _cache[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _act_device(e, obs, eps, step=0, sync=True):
    """act_sample_device on host arrays (float32 or uint8 frames): (action, clipped, logp) as numpy, or the device tensors"""
    n = obs.shape[0]
    o = _dev(obs)
    ep = _dev(eps) if eps is not None else None
    act = torch.empty(n, e.act_dim, device="cuda")
    clip, lp = torch.empty_like(act), torch.empty(n, device="cuda")
    torch.cuda.synchronize()                       # the inputs were produced on torch's stream; the call runs on the engine's
    e.act_sample_device(o, ep, step, act, clip, lp)
    if not sync:
        return act, clip, lp, o, ep
    e.sync()
    return act.cpu().numpy(), clip.cpu().numpy(), lp.cpu().numpy()


def _act_mode(e, obs):
    o, act = _dev(obs), torch.empty(obs.shape[0], e.act_dim, device="cuda")
    torch.cuda.synchronize()
    e.act_mode_device(o, act)
    e.sync()
    return act.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _quiet(e):
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


# ---- stage A: fp32 frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 64, 70])
@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_injected_eps_is_bitwise_the_batch_call(shape, A, ct, n):
    alg, _, obs, eps, (ra, rlp) = _shared(shape, A, ct)
    e = alg.engine
    calls = e.debug_get("act_dev_calls")
    a, c, lp = _act_device(e, obs[:n], eps[:n])
    assert e.debug_get("act_dev_calls") - calls == -(-n // 64)        # chunks of 64 frames
    assert np.array_equal(_bits(a), _bits(ra[:n])) and np.array_equal(_bits(lp), _bits(rlp[:n])), n
    assert np.array_equal(_bits(c), _bits(np.clip(a, e.act_low, e.act_high)))
    a2, c2, lp2 = _act_device(e, obs[:n].reshape(n, -1), eps[:n])    # [n, O] rows are the same frames
    assert np.array_equal(_bits(a), _bits(a2)) and np.array_equal(_bits(c), _bits(c2)) and np.array_equal(_bits(lp), _bits(lp2))
    _quiet(e)


@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_drawn_noise_does_not_depend_on_the_batch_or_the_chunk(shape, A, ct):
    alg, _, obs, _, _ = _shared(shape, A, ct)
    e = alg.engine
    e.set_act_rng(0x1234567887654321)
    big = _act_device(e, obs, None, 3)                                 # 70 frames: a full chunk and a second one
    small = _act_device(e, obs[:4], None, 3)
    for x, y in zip(big, small):
        assert np.array_equal(_bits(x[:4]), _bits(y))
    other = np.concatenate([obs[6:70], obs[64:70]])                     # the same six frames at rows 64..69 of another batch
    for x, y in zip(big, _act_device(e, other, None, 3)):
        assert np.array_equal(_bits(x[64:]), _bits(y[64:]))
    assert not np.array_equal(big[0], _act_device(e, obs, None, 4)[0])  # the step reaches the counter
    _quiet(e)


# ---- stage B: byte frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 70])
@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_byte_frames_act_bit_for_bit_like_their_decoded_frames(shape, A, ct, n):
    alg, codes, obs, eps, _ = _shared(shape, A, ct)
    e = alg.engine
    calls = e.debug_get("act_dev_calls")
    want = _act_device(e, obs[:n], eps[:n])
    got = _act_device(e, codes[:n], eps[:n])
    assert e.debug_get("act_dev_calls") - calls == 2 * -(-n // 64)
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w)), n
    flat = _act_device(e, codes[:n].reshape(n, -1), eps[:n])
    assert all(np.array_equal(_bits(g), _bits(f)) for g, f in zip(got, flat))
    e.set_act_rng(77)
    for g, w in zip(_act_device(e, codes[:n], None, 9), _act_device(e, obs[:n], None, 9)):     # drawn noise too
        assert np.array_equal(_bits(g), _bits(w)), n
    _quiet(e)


# ---- the ring ----------------------------------------------------------------------------------------------------------------------
def _transitions(shape, A, n, rng):
    codes, codes2 = (rng.integers(0, 256, (n,) + tuple(shape), dtype=np.uint8) for _ in range(2))
    return {"codes": codes, "codes2": codes2, "act": rng.standard_normal((n, A)).astype(np.float32),
            "rew": rng.standard_normal(n).astype(np.float32), "term": rng.random(n) < 0.3, "trunc": rng.random(n) < 0.3,
            "logp": rng.standard_normal(n).astype(np.float32)}


def _add_device(e, t, byte_frames, scale):
    img = (lambda c: _dev(c)) if byte_frames else (lambda c: _dev(BOOK[c]))
    cols = (img(t["codes"]), _dev(t["act"]), _dev(t["rew"]), img(t["codes2"]), _dev(t["term"]), _dev(t["trunc"]), _dev(t["logp"]))
    torch.cuda.synchronize()
    e.buffer_add_device(*cols, reward_scale=scale)
    return cols       # (kept alive by the caller until the stream has consumed them)


def _store(ref, t, scale):
    """the reference's store() with the sampler's bookkeeping; returns the rows as dsact_buffer_add takes them"""
    n = t["rew"].shape[0]
    obs, obs2 = BOOK[t["codes"]].reshape(n, -1), BOOK[t["codes2"]].reshape(n, -1)
    row0 = ref.ptr
    for i in range(n):
        ref.store(obs[i], t["act"][i], scale * float(t["rew"][i]), obs2[i], bool(t["term"][i]) and not bool(t["trunc"][i]), t["logp"][i])
    rows = (row0 + np.arange(n)) % ref.cap
    return obs, t["act"], ref.buf["rew"][rows].copy(), obs2, ref.buf["done"][rows].copy(), t["logp"]


def _ring_equals(e, ref, coded):
    got = e.buffer_export(0, ref.size)
    for k in ("obs", "obs2"):
        want = ref.buf[k][:ref.size]
        if coded:
            assert got[k].dtype == np.uint8 and np.array_equal(got[k].reshape(ref.size, -1), np.rint(want * 255).astype(np.uint8)), k
        else:
            assert np.array_equal(_bits(got[k].reshape(ref.size, -1)), _bits(want)), k
    for k in ("act", "rew", "done", "logp"):
        assert np.array_equal(_bits(got[k].reshape(ref.size, -1)), _bits(ref.buf[k][:ref.size].reshape(ref.size, -1))), k


RING_CASES = [pytest.param((3, 96, 96), 3, "type_2", 1, id="type_2-scale1"), pytest.param((3, 96, 96), 3, "type_2", 0.25, id="type_2-scale0.25"),
              pytest.param((4, 84, 84), 2, "type_1", 0.25, id="type_1-scale0.25")]


@pytest.mark.parametrize("coded", [False, True], ids=["fp32", "coded"])
@pytest.mark.parametrize("shape,A,ct,scale", RING_CASES)
def test_ring_rows_equal_the_reference_store_after_wrapping(shape, A, ct, scale, coded):
    book = BOOK if coded else None
    e = _make(shape, A, ct, book=book)[0].engine
    host = _make(shape, A, ct, book=book)[0].engine                   # the same rows through dsact_buffer_add
    cap, O = 40, int(np.prod(shape))
    ref = _HostRing(cap, O, A)
    rng = np.random.default_rng(11)
    for rnd in range(6):                                                # 72 transitions into 40 rows: the ring wraps
        t = _transitions(shape, A, 12, rng)
        keep = _add_device(e, t, False, scale)
        host.buffer_add(*_store(ref, t, scale))
        assert (e.buffer_ptr, e.buffer_size) == (ref.ptr, ref.size) == ((rnd + 1) * 12 % cap, min((rnd + 1) * 12, cap)), rnd
        assert e.debug_get("ring_commit_rows") == (rnd + 1) * 12
        _ring_equals(e, ref, coded)
        del keep
    e.buffer_check()
    assert tuple(e.buffer_digest()) == tuple(host.buffer_digest())
    _quiet(e)


@pytest.mark.parametrize("shape,A,ct,scale", RING_CASES)
def test_byte_rows_fill_the_coded_ring_like_their_decoded_frames(shape, A, ct, scale):
    e = _make(shape, A, ct, book=BOOK)[0].engine
    f = _make(shape, A, ct, book=BOOK)[0].engine                      # BOOK[b] as fp32 through buffer_add_device
    cap, O = 40, int(np.prod(shape))
    ref = _HostRing(cap, O, A)
    rng = np.random.default_rng(12)
    for rnd in range(6):
        t = _transitions(shape, A, 12, rng)
        keep = _add_device(e, t, True, scale), _add_device(f, t, False, scale)
        _store(ref, t, scale)
        assert (e.buffer_ptr, e.buffer_size) == (ref.ptr, ref.size), rnd
        _ring_equals(e, ref, True)
        del keep
    e.buffer_check()
    assert tuple(e.buffer_digest()) == tuple(f.buffer_digest())
    _quiet(e)


def test_a_byte_outside_the_codebook_is_reported_like_an_encoder_miss():
    from dsact._ffi import DsactError

    shape, A, ct = (3, 96, 96), 3, "type_2"
    e = _make(shape, A, ct, book=BOOK[:200])[0].engine
    rng = np.random.default_rng(13)
    keep = []
    for rnd in range(3):
        t = _transitions(shape, A, 12, rng)
        t["codes"], t["codes2"] = (t["codes"] % 200).astype(np.uint8), (t["codes2"] % 200).astype(np.uint8)
        if rnd == 2:
            t["codes2"][7, 1, 50, 33] = 231                             # transition 7 of the third add: ring row 31
        keep.append(_add_device(e, t, True, 1))
    with pytest.raises(DsactError, match=r"E_INVALID.*hip_obs_codebook: 1 observation.*first recorded: 231 .*ring row 31"):
        e.buffer_check()
    assert e.buffer_size == 36 and e.buffer_ptr == 36
    with pytest.raises(DsactError, match="not in the codebook"):
        _add_device(e, _transitions(shape, A, 4, rng), True, 1)
    assert e.buffer_size == 36


def test_byte_frames_need_a_coded_ring():
    from dsact._ffi import DsactError

    shape, A, ct = (3, 96, 96), 3, "type_2"
    e = _make(shape, A, ct, book=None)[0].engine
    t = _transitions(shape, A, 4, np.random.default_rng(1))
    eps = np.zeros((4, A), np.float32)
    with pytest.raises(DsactError, match="E_STATE.*hip_obs_codebook"):
        _act_device(e, t["codes"], eps)
    with pytest.raises(DsactError, match="E_STATE.*hip_obs_codebook"):
        _act_mode(e, t["codes"])
    with pytest.raises(DsactError, match="E_STATE.*hip_obs_codebook"):
        _add_device(e, t, True, 1)
    assert e.buffer_size == 0
    # ... and the handle works
    a = _act_device(e, BOOK[t["codes"]], eps)[0]
    _add_device(e, t, False, 1)
    e.sync()
    assert e.buffer_size == 4 and np.isfinite(a).all()
    _quiet(e)


# ---- the event behind a device-resident call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_held_call_after_a_device_call_waits_for_its_launches(shape, A, ct):
    alg, _, obs, eps, _ = _shared(shape, A, ct)
    e = alg.engine
    rng = np.random.default_rng(21)
    obs5 = rng.uniform(0.0, 1.0, (5,) + tuple(shape)).astype(np.float32)
    eps5 = rng.standard_normal((5, A)).astype(np.float32)

    def both(sync_between):
        out = _act_device(e, obs, eps, sync=False)
        if sync_between:
            e.sync()
        e.behaviour_hold()
        held = e.act_sample_batch(obs5, eps5)
        e.sync()
        e.behaviour_release()
        return [t.cpu().numpy() for t in out[:3]] + [held[0].copy(), held[1].copy()]

    want, got = both(True), both(False)
    for w, g in zip(want, got):
        assert np.array_equal(_bits(w), _bits(g))
    _quiet(e)


# ---- stage C: the mode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 70])
@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_mode_equals_the_module_forward_and_bytes_equal_frames(shape, A, ct, n):
    alg, codes, obs, _, _ = _shared(shape, A, ct)
    e = alg.engine
    if ("twin",) + (shape,) not in _cache:
        _cache[("twin",) + (shape,)] = _cpu_twin(alg, _kw(shape, A, ct))
    ref = _cache[("twin",) + (shape,)]
    calls = e.debug_get("act_mode_dev_calls")
    a = _act_mode(e, obs[:n])
    assert e.debug_get("act_mode_dev_calls") - calls == -(-n // 64)
    ra, rlp, rlg = _reference(ref, obs[:n], np.zeros((n, A), np.float32))   # eps = 0: the sample IS the mode
    print("n=%d max |mode - ref| = %.3g" % (n, np.abs(a - ra).max()))
    _check(a, rlp, ra, rlp, rlg, LIM, False, (ct, n))
    assert np.array_equal(_bits(_act_mode(e, codes[:n])), _bits(a))
    assert np.array_equal(_bits(_act_mode(e, obs[:n].reshape(n, -1))), _bits(a))
    _quiet(e)


# ---- the classes -------------------------------------------------------------------------------------------------------------------
def _train(tmp, name, frames):
    import plugin
    from synth_tensor_blob import SynthTensorBlob
    from training.hip_trainer import HipOffSerialTrainer, read_scalars

    shape, A, N, S, K, iters, cap, warm = (3, 96, 96), 3, 8, 8, 8, 16, 64, 16
    folder = str(tmp / name)
    kw = _kw(shape, A, "type_2", buffer_max_size=cap, buffer_warm_size=warm, seed=3, sample_batch_size=S, sample_interval=K,
             max_iteration=iters, log_save_interval=8, apprfunc_save_interval=100000, eval_interval=100000, save_folder=folder,
             ini_network_dir=None, hip_device_indices=True, reward_scale=0.25, sampler_name="hip_tensor_env_sampler")
    if frames == "uint8":
        kw["hip_obs_codebook"] = BOOK
    torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    e = alg.engine
    assert buf.engine is e and e.cnn_act
    smp = plugin.create_sampler(env=SynthTensorBlob(N, device="cuda", seed=4, frames=frames), **kw)
    adds, inner = [], buf.add_batch

    def add_batch(batch):
        e.sync()
        assert batch.obs.dtype == getattr(torch, frames) and tuple(batch.obs.shape) == (S,) + shape
        adds.append([c.cpu().numpy().copy() for c in batch.device_columns])
        inner(batch)

    buf.add_batch = add_batch
    tr = plugin.create_trainer(alg, smp, buf, None, **kw)
    assert type(tr) is HipOffSerialTrainer
    tr.train()
    e.sync()
    n_samples = warm // S * S + (iters + K - 1) // K * S
    assert smp.get_total_sample_number() == n_samples and smp.act_step == n_samples // N and len(adds) == n_samples // S
    assert buf.size == min(n_samples, cap) and buf.ptr == n_samples % cap
    assert e.debug_get("ring_commit_rows") == n_samples and e.debug_get("act_batch_calls") == 0.0
    _quiet(e)
    scal = read_scalars(folder)
    assert len(scal["Loss/Critic loss-RL iter"]["y"]) == iters // 8
    stats = {tag: np.asarray(d["y"]) for tag, d in scal.items() if not tag.startswith(("Time/", "RAM/"))}
    for tag, y in stats.items():
        assert np.isfinite(y).all(), tag
    assert torch.isfinite(e.online).all()
    return {"adds": adds, "digest": tuple(e.buffer_digest()), "stats": stats, "warm_adds": warm // S}


@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_serial_trainer_runs_on_the_image_sampler_and_repeats_bitwise(tmp_path, frames):
    a, b = _train(tmp_path, "a", frames), _train(tmp_path, "b", frames)
    assert a["digest"] == b["digest"] and a["stats"].keys() == b["stats"].keys()
    for tag in a["stats"]:
        assert np.array_equal(a["stats"][tag], b["stats"][tag]), tag
    _cache[("loop", frames)] = a
    if ("loop", "float32") in _cache and ("loop", "uint8") in _cache:
        # the byte run's rows, decoded, are the fp32 run's through the first sample() of the loop (no update has run before it)
        f, u = _cache[("loop", "float32")], _cache[("loop", "uint8")]
        for k in range(f["warm_adds"] + 1):
            for j, (x, y) in enumerate(zip(f["adds"][k], u["adds"][k])):
                y = BOOK[y] if j in (0, 3) else y
                assert np.array_equal(x, y), (k, j)


@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_evaluator_returns_equal_stepping_the_environment_by_hand(frames):
    from synth_tensor_blob import SynthTensorBlob
    from training.hip_tensor_evaluator import HipTensorEnvEvaluator

    shape, A, ct = (3, 96, 96), 3, "type_2"
    alg = _shared(shape, A, ct)[0]
    e = alg.engine
    N, E = 4, 3
    ev = HipTensorEnvEvaluator(env=SynthTensorBlob(N, device="cuda", seed=6, frames=frames), networks=alg.networks,
                               num_eval_episode=E, hip_cnn_act=True, hip_eval_poll_steps=5)
    calls = e.debug_get("act_mode_dev_calls")
    mean = ev.run_evaluation(0)
    assert e.debug_get("act_mode_dev_calls") - calls == ev.steps == 20
    # by hand: row i plays episode i; every step's action from act_mode_device, the returns summed in float64 in step order
    env = SynthTensorBlob(N, device="cuda", seed=6, frames=frames)
    obs = env.reset()
    ret, length, returns, lengths = np.zeros(N), np.zeros(N, np.int32), [None] * E, [None] * E
    act = torch.empty(N, A, device="cuda")
    for _ in range(20):
        torch.cuda.synchronize()
        e.act_mode_device(obs.contiguous(), act)
        e.sync()
        obs2, r, te, tr = env.step(act)
        ret += r.cpu().numpy().astype(np.float64)
        length += 1
        ended = (te | tr).cpu().numpy()
        for i in np.flatnonzero(ended):
            if i < E and returns[i] is None:
                returns[i], lengths[i] = ret[i], length[i]
        obs = env.reset(te | tr)
    assert np.array_equal(ev.returns, np.asarray(returns, np.float64)) and np.array_equal(ev.lengths, np.asarray(lengths, np.int32))
    assert mean == np.mean(ev.returns) and list(ev.lengths) == [20] * E
    _quiet(e)


# ---- nothing waited, host pointers are refused ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_no_waits_and_host_pointers_are_refused(shape, A, ct):
    alg, codes, obs, eps, _ = _shared(shape, A, ct)
    e = alg.engine
    _quiet(e)
    n, O = 4, int(np.prod(shape))
    f = lambda *s: torch.zeros(*s, device="cuda")
    d_obs, act, clip, lp = _dev(obs[:n]), f(n, A), f(n, A), f(n)
    d_codes, flags = _dev(codes[:n]), torch.zeros(n, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    h_obs, h_codes, h_out = np.ascontiguousarray(obs[:n]), np.ascontiguousarray(codes[:n]), np.zeros((n, A), np.float32)
    pinned = torch.zeros(n, O).pin_memory()
    P = lambda t: C.c_void_p(t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr())
    lib, h = e._lib, e._h
    e.set_act_rng(9)
    size = e.buffer_size
    for bad in (h_obs, pinned):
        assert lib.dsact_act_sample_device(h, P(bad), n, None, 0, P(act), P(clip), P(lp)) == -1
        assert b"device pointers" in lib.dsact_last_error(h)
        assert lib.dsact_act_mode_device(h, P(bad), n, P(act)) == -1
        assert b"device pointers" in lib.dsact_last_error(h)
    assert lib.dsact_act_sample_device_u8(h, P(h_codes), n, None, 0, P(act), P(clip), P(lp)) == -1
    assert b"device pointers" in lib.dsact_last_error(h)
    assert lib.dsact_act_mode_device_u8(h, P(d_codes), n, P(h_out)) == -1
    assert b"device pointers" in lib.dsact_last_error(h)
    assert lib.dsact_buffer_add_device(h, n, P(h_obs), P(act), P(lp), P(d_obs), P(flags), P(flags), P(lp), 1.0) == -1
    assert b"device pointers" in lib.dsact_last_error(h)
    assert lib.dsact_buffer_add_device_u8(h, n, P(d_codes), P(act), P(lp), P(h_codes), P(flags), P(flags), P(lp), 1.0) == -1
    assert b"device pointers" in lib.dsact_last_error(h) and e.buffer_size == size
    with pytest.raises(ValueError, match="dtype"):
        e.act_sample_device(d_obs.double(), None, 0, act, clip, lp)
    with pytest.raises(ValueError, match="shape"):
        e.act_sample_device(d_obs[:, :, :-1].contiguous(), None, 0, act, clip, lp)
    with pytest.raises(ValueError, match="same dtype"):
        e.buffer_add_device(d_obs, act, lp, d_codes, flags, flags, lp)
    # ... and the handle works
    e.act_sample_device(d_obs, None, 0, act, clip, lp)
    e.buffer_add_device(d_codes, act, lp, d_codes, flags, flags, lp, 0.5)
    e.sync()
    assert e.buffer_size == min(size + n, 40) and torch.isfinite(act).all()
    _quiet(e)
