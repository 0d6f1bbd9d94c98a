"""Image tensor environments inside the sample / eval graphs on the GPU (dsact_cnn_acting_capture, dsact_act_sample_device_counted /
_u8 on a CNN handle, dsact_step_frames_device / k_step_frames, training/hip_tensor_sampler.py and hip_tensor_evaluator.py with
hip_graph_* = True and hip_cnn_act=True). Everything is compared BITWISE: the captured route runs the
kernels of the eager route on the same inputs.

  1. dsact_step_frames_device == the torch copies and the `|`, on each of its three access paths, with the bytes around every
     slot intact;
  2. a CNN handle without the opt-in refuses the counted forms and a capture as it always did; the opt-in's own rules;
  3. on an opted-in handle hand-made graphs of the mode call and of the counted call (+ counter_add) replay to the eager bits,
     for both shapes, both frame dtypes, one chunk and two; the host-call counters move at capture time only;
  4. a held call after replays returns the bits of the same call on a handle that never captured (the fence it records itself);
  5. the sampler with both kwargs on the in-place fixture == the eager sampler on the plain fixture, on twin engines;
  6. a replay reads the weights a local_update left in the arena;
  7. the evaluator likewise;
  8. HipOffSerialTrainer with both graph kwargs ends bitwise equal to the run with neither.

Shapes: (3, 96, 96) type_2 with A = 3 takes the RGB ingest forms, (4, 84, 84) type_1 with A = 2 the generic form; n = 5 is one
chunk with a ragged last workgroup, n = 70 two chunks (64 + 6). Handles are built at batch 16.

Two rules of the library cannot be reached from here and are not asserted: "make one call outside the capture first" -- on an
enabled CNN handle dsact_cnn_acting_enable has made every allocation of the forward, so a capture may be the handle's first acting
call (asserted below) -- and "while profiling", a state that exists only inside dsact_profile_step.
"""
import os
import sys

import numpy as np
import pytest
import torch

from test_tensor_image_gpu import BOOK, _kw, _make

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

SHAPES = [pytest.param((4, 84, 84), 2, "type_1", id="type_1"), pytest.param((3, 96, 96), 3, "type_2", id="type_2")]
BLOB, BLOB_A, BLOB_CT = (3, 96, 96), 3, "type_2"
PER_DIM = {"mean": [-0.05, 0.0, 0.05], "std": [0.02, 0.1, 0.2]}
_cache = {}


def _bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    t = np.ascontiguousarray(t)
    return t.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[t.dtype.itemsize])


def _quiet(e):
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


def _opted(shape, A, ct):
    """(engine with a coded ring and the opt-in, codes[70], frames[70] = BOOK[codes] on the device): built once per shape"""
    key = ("opted", shape)
    if key not in _cache:
        e = _make(shape, A, ct, book=BOOK)[0].engine
        e.cnn_acting_capture()
        assert e.debug_get("cnn_act_capture") == 1.0
        e.set_act_rng(0x1234567887654321)
        codes = np.random.default_rng(7).integers(0, 256, (70,) + tuple(shape), dtype=np.uint8)
        _cache[key] = (e, torch.from_numpy(codes).cuda(), torch.from_numpy(BOOK[codes]).cuda())
        torch.cuda.synchronize()
    return _cache[key]


def _outs(n, A):
    return [torch.full((n, A), float("nan"), device="cuda"), torch.full((n, A), float("nan"), device="cuda"),
            torch.full((n,), float("nan"), device="cuda")]


def _refusals_under_capture(e, calls):
    from dsact._ffi import DsactError

    g = torch.cuda.CUDAGraph()
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


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
# (row bytes, byte offset of source and slot inside their 256-byte aligned allocations, the access path)
FRAME_CASES = [pytest.param(27648, 0, 2, id="u8-3x96x96"), pytest.param(28224, 0, 2, id="u8-4x84x84"),
               pytest.param(110592, 0, 2, id="fp32-3x96x96"), pytest.param(20, 0, 1, id="20-bytes"), pytest.param(7, 0, 0, id="7-bytes"),
               pytest.param(27648, 4, 1, id="16-aligned-size-at-a-4-aligned-offset")]


@pytest.mark.parametrize("row_bytes,offset,path", FRAME_CASES)
def test_step_frames_equal_the_torch_copies(row_bytes, offset, path):
    e = _opted(BLOB, BLOB_A, BLOB_CT)[0]
    g = torch.Generator(device="cuda").manual_seed(9)
    guard = 256                                                         # bytes kept on either side of everything written
    for n in (1, 5, 70):
        size = n * row_bytes
        assert (row_bytes % 16 == 0 and offset % 16 == 0) == (path == 2) and (row_bytes % 4 == 0 and offset % 4 == 0) == (path >= 1)
        src_buf = torch.randint(0, 256, (offset + size,), dtype=torch.uint8, device="cuda", generator=g)
        # the slot is rows [n, 2n) of a [3n, row_bytes] block that starts `offset` bytes into its allocation
        dst_buf = torch.randint(0, 256, (guard + offset + 3 * size + guard,), dtype=torch.uint8, device="cuda", generator=g)
        assert src_buf.data_ptr() % 256 == 0 and dst_buf.data_ptr() % 256 == 0
        lo = guard + offset + size
        obs2, slot = src_buf[offset:offset + size].view(n, row_bytes), dst_buf[lo:lo + size].view(n, row_bytes)
        if row_bytes == 110592:                                         # the same bytes as fp32 frames: the element type is no part of it
            obs2, slot = obs2.view(torch.float32).view(n, 3, 96, 96), slot.view(torch.float32).view(n, 3, 96, 96)
        rew = torch.randn(n, device="cuda", generator=g)
        term, trunc = (torch.rand(n, device="cuda", generator=g) < 0.3 for _ in range(2))
        got = [torch.full((3 * n,), -3.25, device="cuda"), torch.zeros(3 * n, dtype=torch.bool, device="cuda"),
               torch.ones(3 * n, dtype=torch.bool, device="cuda")]
        want = [t.clone() for t in got]
        for dst, src in zip(want, (rew, term, trunc)):
            dst[n:2 * n].copy_(src)
        want_buf = dst_buf.clone()
        want_buf[lo:lo + size].copy_(src_buf[offset:offset + size])
        ended = torch.zeros(n + 2, dtype=torch.bool, device="cuda")      # a guard byte on either side
        torch.cuda.synchronize()
        calls = e.debug_get("step_frames_calls")
        e.step_frames_device(obs2, rew, term, trunc, slot, *(t[n:2 * n] for t in got), ended[1:n + 1])
        e.sync()
        assert e.debug_get("step_frames_calls") - calls == 1
        assert torch.equal(dst_buf, want_buf), (n, "frames and the bytes around the slot")
        for k, (u, v) in enumerate(zip(got, want)):
            assert np.array_equal(_bits(u), _bits(v)), (n, k)
        assert torch.equal(ended[1:n + 1], term | trunc) and not bool(ended[0]) and not bool(ended[n + 1]), n
        if n > 1:
            assert bool(ended.any()) and not bool(ended[1:n + 1].all())
    _quiet(e)
    with pytest.raises(ValueError):                                     # rows that are not contiguous
        e.step_frames_device(obs2.reshape(n, -1)[:, ::2], rew, term, trunc, slot.reshape(n, -1)[:, ::2], *(t[n:2 * n] for t in got), ended[1:n + 1])


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def test_a_handle_without_the_opt_in_answers_as_it_always_did():
    from dsact._ffi import DsactError

    alg, _ = _make(BLOB, BLOB_A, BLOB_CT, book=BOOK)
    e = alg.engine
    n = 5
    assert e.debug_get("cnn_act_capture") == 0.0
    e.set_act_rng(5)
    e.act_counter_set(0)
    codes = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (n,) + BLOB, dtype=np.uint8)).cuda()
    frames = torch.from_numpy(BOOK).cuda()[codes.to(torch.int64)]
    act, clip, lp = _outs(n, BLOB_A)
    torch.cuda.synchronize()
    for obs in (frames, codes):
        with pytest.raises(DsactError, match=r"E_INVALID.*serves MLP policies \(the CNN route records an event per call\)"):
            e.act_sample_device_counted(obs, 0, act, clip, lp)
    e.act_mode_device(frames, act)
    e.sync()
    want = act.clone()
    refused = _refusals_under_capture(e, [lambda: e.act_mode_device(frames, act), lambda: e.act_mode_device(codes, act)])
    assert all(r is not None and "E_INVALID" in r and "under stream capture serves MLP policies" in r for r in refused), refused
    act.fill_(float("nan"))
    e.act_mode_device(codes, act)                                       # the handle is usable
    e.sync()
    assert np.array_equal(_bits(act), _bits(want))
    # the opt-in's own rules: not under capture, not on a handle without the acting path, and it cannot be taken back
    refused = _refusals_under_capture(e, [e.cnn_acting_capture])
    assert refused[0] is not None and "E_STATE" in refused[0] and e.debug_get("cnn_act_capture") == 0.0
    assert e._lib.dsact_cnn_acting_capture(e._h, 0) == 0                 # off while off: nothing happens
    e.cnn_acting_capture()
    e.cnn_acting_capture()                                              # idempotent
    assert e.debug_get("cnn_act_capture") == 1.0
    assert e._lib.dsact_cnn_acting_capture(e._h, 0) != 0 and e.debug_get("cnn_act_capture") == 1.0
    e.act_sample_device_counted(codes, 0, act, clip, lp)                # ... and now the counted forms serve the handle
    e.act_sample_device_counted(frames, 0, *_outs(n, BLOB_A))
    e.sync()
    assert torch.isfinite(act).all()
    with pytest.raises(DsactError, match="E_INVALID.*16-byte aligned"):
        e.act_sample_device_counted(torch.zeros(n * 27648 + 1, device="cuda")[1:].view((n,) + BLOB), 0, act, clip, lp)
    _quiet(e)
    from helpers import hip_kwargs
    import plugin
    torch.manual_seed(1)
    mlp = plugin.create_alg(**hip_kwargs(17, 6, (64, 64), 64, strict_rng=False)).engine
    with pytest.raises(DsactError, match="E_STATE.*dsact_cnn_acting_enable"):
        mlp.cnn_acting_capture()


def test_byte_frames_under_the_opt_in_still_need_a_coded_ring_and_a_capture_may_be_the_first_acting_call():
    from dsact._ffi import DsactError

    e = _make(BLOB, BLOB_A, BLOB_CT, book=None)[0].engine               # an fp32 ring: no codebook
    e.cnn_acting_capture()
    e.set_act_rng(5)
    n = 5
    codes = torch.zeros((n,) + BLOB, dtype=torch.uint8, device="cuda")
    frames = torch.rand((n,) + BLOB, device="cuda")
    act, clip, lp = _outs(n, BLOB_A)
    torch.cuda.synchronize()
    # the counted form before dsact_act_counter_set is a state error, under capture as outside it
    refused = _refusals_under_capture(e, [lambda: e.act_sample_device_counted(frames, 0, act, clip, lp)])
    assert refused[0] is not None and "E_STATE" in refused[0] and "dsact_act_counter_set" in refused[0]
    e.act_counter_set(3)
    with pytest.raises(DsactError, match="E_STATE.*hip_obs_codebook"):
        e.act_sample_device_counted(codes, 0, act, clip, lp)
    refused = _refusals_under_capture(e, [lambda: e.act_mode_device(codes, act)])
    assert refused[0] is not None and "E_STATE" in refused[0] and "hip_obs_codebook" in refused[0]
    # dsact_cnn_acting_enable made every allocation of the forward: the handle's FIRST acting call may be a captured one
    assert e.debug_get("act_mode_dev_calls") == 0.0 and e.debug_get("act_dev_calls") == 0.0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=e.torch_stream, capture_error_mode="relaxed"):
        e.act_mode_device(frames, act)
    with torch.cuda.stream(e.torch_stream):
        g.replay()
    e.sync()
    got = act.clone()
    e.act_mode_device(frames, act)
    e.sync()
    assert torch.isfinite(got).all() and np.array_equal(_bits(got), _bits(act))
    _quiet(e)
    del g


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 70])
@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_hand_made_graphs_replay_to_the_eager_bits(shape, A, ct, n):
    e, codes, frames = _opted(shape, A, ct)
    chunks = -(-n // 64)
    for obs in (codes[:n], frames[:n]):
        # the mode call
        act = _outs(n, A)[0]
        e.act_mode_device(obs, act)
        e.sync()
        want = act.clone()
        assert torch.isfinite(want).all()
        act.fill_(float("nan"))
        torch.cuda.synchronize()
        calls = e.debug_get("act_mode_dev_calls")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=e.torch_stream, capture_error_mode="relaxed"):
            e.act_mode_device(obs, act)
        assert e.debug_get("act_mode_dev_calls") - calls == chunks       # host calls: counted at capture time
        e.sync()
        assert bool(torch.isnan(act).all())                             # captured, not run
        for _ in range(2):
            with torch.cuda.stream(e.torch_stream):
                g.replay()
            e.sync()
            assert np.array_equal(_bits(act), _bits(want)), (obs.dtype, "mode")
            act.fill_(float("nan"))
            torch.cuda.synchronize()
        assert e.debug_get("act_mode_dev_calls") - calls == chunks       # ... and not when it is replayed
        del g
        # the counted call and the node that closes a sample(): replay k draws the noise of steps c + 1 + 2 k
        c = 2 ** 32 - 3
        e.act_counter_set(c)
        out, ref = _outs(n, A), _outs(n, A)
        torch.cuda.synchronize()
        calls = e.debug_get("act_dev_calls")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=e.torch_stream, capture_error_mode="relaxed"):
            e.act_sample_device_counted(obs, 1, *out)
            e.act_counter_add(2)
        assert e.debug_get("act_dev_calls") - calls == chunks
        assert e.act_counter_read() == c and bool(torch.isnan(out[0]).all())
        seen = []
        for k in range(3):                                              # steps 2^32 - 2, 2^32, 2^32 + 2: across the carry
            with torch.cuda.stream(e.torch_stream):
                g.replay()
            e.sync()
            assert e.debug_get("act_dev_calls") - calls == chunks + k * chunks   # (only the eager reference calls below add to it)
            e.act_sample_device(obs, None, c + 1 + 2 * k, *ref)
            e.sync()
            for x, y, name in zip(out, ref, ("action", "clipped", "logp")):
                assert np.array_equal(_bits(x), _bits(y)), (obs.dtype, k, name)
            seen.append(out[0].clone())
        assert e.act_counter_read() == c + 6
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])   # every replay drew its own step's noise
        del g
    _quiet(e)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_held_call_after_replays_equals_the_call_on_a_handle_that_never_captured(shape, A, ct):
    e, codes, frames = _opted(shape, A, ct)
    twin = _make(shape, A, ct, book=BOOK)[0].engine                      # the same seed: the same weights, no opt-in, no capture
    assert torch.equal(twin.online, e.online) and twin.debug_get("cnn_act_capture") == 0.0
    rng = np.random.default_rng(21)
    obs5 = rng.uniform(0.0, 1.0, (5,) + tuple(shape)).astype(np.float32)
    eps5 = rng.standard_normal((5, A)).astype(np.float32)
    twin.behaviour_hold()
    want = twin.act_sample_batch(obs5, eps5)
    twin.behaviour_release()
    want = (want[0].copy(), want[1].copy())
    e.act_counter_set(0)
    out = _outs(70, A)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=e.torch_stream, capture_error_mode="relaxed"):
        e.act_sample_device_counted(codes, 0, *out)
        e.act_sample_device_counted(frames, 1, *out)
        e.act_counter_add(2)
    e.behaviour_hold()
    with torch.cuda.stream(e.torch_stream):
        for _ in range(4):                                              # the path's buffers are busy on the handle's stream ...
            g.replay()
    held = e.act_sample_batch(obs5, eps5)                               # ... when the held call starts on the acting stream
    held = (held[0].copy(), held[1].copy())
    e.sync()
    e.behaviour_release()
    assert np.array_equal(_bits(held[0]), _bits(want[0])) and np.array_equal(_bits(held[1]), _bits(want[1]))
    # ... and the replays computed what they compute without a held call in between
    ref = _outs(70, A)
    e.act_sample_device(frames, None, 7, *ref)
    e.sync()
    for x, y in zip(out, ref):
        assert np.array_equal(_bits(x), _bits(y))
    assert e.act_counter_read() == 8
    _quiet(e)
    del g


# ---- 5, 6 ----------------------------------------------------------------------------------------------------------------------
def _twins(frames, key="twins"):
    """((alg, buffer) eager, (alg, buffer) graph): two handles with the same weights and rings, built once per frame dtype"""
    if (key, frames) not in _cache:
        book = BOOK if frames == "uint8" else None
        pair = _make(BLOB, BLOB_A, BLOB_CT, cap=160, book=book), _make(BLOB, BLOB_A, BLOB_CT, cap=160, book=book)
        assert torch.equal(pair[0][0].engine.online, pair[1][0].engine.online)
        _cache[(key, frames)] = pair
    return _cache[(key, frames)]


def _sampler(alg, graph, frames, N, S, **over):
    import plugin
    from synth_tensor_blob import SynthTensorBlob
    from synth_tensor_blob_inplace import SynthTensorBlobInplace

    env = (SynthTensorBlobInplace if graph else SynthTensorBlob)(N, device="cuda", seed=4, frames=frames)
    more = dict(hip_graph_sample=True) if graph else {}
    more.update(over)
    kw = _kw(BLOB, BLOB_A, BLOB_CT, seed=3, sample_batch_size=S, sampler_name="hip_tensor_env_sampler")
    return plugin.create_sampler(**dict(kw, env=env, networks=alg.networks, **more))


def _take(smp, eng, buf):
    batch, _ = smp.sample()
    eng.sync()
    cols = [t.detach().cpu().clone() for t in batch.device_columns]
    buf.add_batch(batch)
    return cols


def _advance_clock(smp, eng, t):
    """every environment's episode clock -> t, in stream order (the in-place fixture keeps its storage)"""
    with torch.cuda.stream(eng.torch_stream):
        if getattr(smp.env, "capture_safe", False):
            smp.env.t.fill_(t)
        else:
            smp.env.t = torch.full_like(smp.env.t, t)


@pytest.mark.parametrize("variant", ["plain", "noise", "stats", "assign"])
@pytest.mark.parametrize("N,S", [(5, 5), (5, 15), (70, 70)])
@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_sampler_graph_is_bitwise_the_eager_sampler(frames, N, S, variant):
    (alg_e, buf_e), (alg_g, buf_g) = _twins(frames)
    ee, eg = alg_e.engine, alg_g.engine
    for e in (ee, eg):
        e.set_explore_noise(None, None)                                 # (an earlier case may have left it on)
    over = {"noise": dict(noise_params=PER_DIM), "stats": dict(hip_episode_stats=True)}.get(variant, {})
    se, sg = _sampler(alg_e, False, frames, N, S, **over), _sampler(alg_g, True, frames, N, S, **over)
    assert sg.graph_sample and sg.cnn_act and not se.graph_sample
    steps, chunks = S // N, -(-N // 64)
    calls = {k: eg.debug_get(k) for k in ("act_dev_calls", "step_frames_calls")}
    ended = 0
    for call in range(4):                                               # eager, capture (+ its replay), two replays
        if call == 1:
            # 20-step episodes never end in four short calls: move the clocks so that every row is truncated -- and restarted
            # by reset(mask) -- inside the captured body (S = 15) or inside the last replay (S = N)
            for smp, e in ((se, ee), (sg, eg)):
                _advance_clock(smp, e, 17)
        if call == 2 and variant == "assign":
            se.act_step = sg.act_step = 2 ** 32 - 2
            assert eg.act_counter_read() == 2 ** 32 - 2
        be, bg = _take(se, ee, buf_e), _take(sg, eg, buf_g)
        for k, (u, v) in enumerate(zip(be, bg)):
            assert u.dtype == v.dtype and np.array_equal(_bits(u), _bits(v)), (call, k)
        assert be[0].dtype == getattr(torch, frames) and tuple(be[0].shape) == (S,) + BLOB
        ended += int(be[5].sum())
        assert sg.graph_captures == min(call, 1) and sg.graph_replays == call
    assert ended == N, "every row was truncated once, inside the graph"
    eg.sync()
    assert se.act_step == sg.act_step == eg.act_counter_read() == (2 ** 32 - 2 + 2 * steps if variant == "assign" else 4 * steps)
    assert sg.graph_captures == 1 and sg.graph_replays == 3 and se.graph_captures == 0
    assert np.array_equal(_bits(se._obs), _bits(sg._obs))
    assert ee.buffer_digest() == eg.buffer_digest() and any(eg.buffer_digest()) and (buf_e.size, buf_e.ptr) == (buf_g.size, buf_g.ptr)
    # the replays made no library call: the eager and the capturing call issued all there are
    assert eg.debug_get("act_dev_calls") - calls["act_dev_calls"] == 2 * steps * chunks
    assert eg.debug_get("step_frames_calls") - calls["step_frames_calls"] == 2 * steps
    if variant == "stats":
        a, b = se.episode_statistics(), sg.episode_statistics()
        assert a["episodes"] == b["episodes"] == N
        for k in ("terminated_share", "return_mean", "return_min", "return_max", "length_mean"):
            assert a[k] == b[k], k
    assert eg.debug_get("cnn_act_capture") == 1.0 and ee.debug_get("cnn_act_capture") == 0.0
    _quiet(eg)
    _quiet(ee)


def test_a_replay_reads_the_weights_a_local_update_left():
    from oracle.dsact_oracle_cnn import cnn_config, synth_image_batch

    frames, N, S = "float32", 5, 15
    (alg_e, buf_e), (alg_g, buf_g) = _twins(frames, key="update-twins")  # a pair of its own: its weights move
    se, sg = _sampler(alg_e, False, frames, N, S), _sampler(alg_g, True, frames, N, S)
    for call in range(3):
        for u, v in zip(_take(se, alg_e.engine, buf_e), _take(sg, alg_g.engine, buf_g)):
            assert np.array_equal(_bits(u), _bits(v)), call
    ee, eg = alg_e.engine, alg_g.engine
    before = eg.online.clone()
    # what the weights of before would do on the fourth call's first step (step 9: three calls of three steps were made)
    old = _outs(N, BLOB_A)
    with torch.cuda.stream(ee.torch_stream):
        obs = se._obs.clone()
    torch.cuda.synchronize()
    ee.act_sample_device(obs, None, 9, *old)
    ee.sync()
    data = synth_image_batch(cnn_config(BLOB, BLOB_A, BLOB_CT), 16, seed=0)
    for alg in (alg_e, alg_g):
        torch.manual_seed(100)
        alg.local_update(data, 0)
    eg.sync()
    ee.sync()
    assert torch.equal(ee.online, eg.online) and not torch.equal(before, eg.online)
    be, bg = _take(se, ee, buf_e), _take(sg, eg, buf_g)                  # a replay: nothing of it is issued anew
    assert sg.graph_captures == 1 and sg.graph_replays == 3
    for k, (u, v) in enumerate(zip(be, bg)):
        assert np.array_equal(_bits(u), _bits(v)), k
    assert np.array_equal(_bits(bg[0][:N]), _bits(obs))
    assert not np.array_equal(_bits(bg[1][:N]), _bits(old[0]))          # the update did move the actions
    _quiet(eg)


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def _evaluator(alg, graph, frames, N, E, P):
    import plugin
    from synth_tensor_blob import SynthTensorBlob
    from synth_tensor_blob_inplace import SynthTensorBlobInplace

    env = (SynthTensorBlobInplace if graph else SynthTensorBlob)(N, device="cuda", seed=6, frames=frames)
    more = dict(hip_graph_eval=True) if graph else {}
    return plugin.create_evaluator(evaluator_name="hip_tensor_env_evaluator", eval_env=env, num_eval_episode=E, networks=alg.networks,
                                   hip_cnn_act=True, hip_eval_poll_steps=P, **more)


@pytest.mark.parametrize("N,E,P", [(5, 7, 1), (5, 7, 7), (70, 75, 4)])
@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_evaluator_graph_is_bitwise_the_eager_evaluator(frames, N, E, P):
    (alg_e, _), (alg_g, _) = _twins(frames)
    ee, eg = alg_e.engine, alg_g.engine
    eager, graph = _evaluator(alg_e, False, frames, N, E, P), _evaluator(alg_g, True, frames, N, E, P)
    assert graph.graph_eval and graph.cnn_act and not eager.graph_eval
    need = 20 * -(-E // N)                                              # every episode is 20 steps; the busiest row plays ceil(E / N)
    windows = -(-need // P)
    modes = eg.debug_get("act_mode_dev_calls")
    for run in range(3):
        tar_e, tar_g = eager.run_evaluation(run), graph.run_evaluation(run)
        assert np.array_equal(_bits(np.array([tar_e])), _bits(np.array([tar_g]))), run       # the TAR's bits
        assert np.array_equal(_bits(eager.returns), _bits(graph.returns)) and np.array_equal(eager.lengths, graph.lengths), run
        assert eager.steps == graph.steps == windows * P, run
    assert np.isfinite(graph.returns).all() and list(graph.lengths) == [20] * E and len(set(graph.returns.tolist())) > 1
    assert graph.graph_captures == 1 and graph.graph_replays == 3 * windows - 1     # one capture, then a replay per full window
    assert eager.graph_captures == 0 and eager.graph_replays == 0
    assert eg.debug_get("act_mode_dev_calls") - modes == 2 * P * -(-N // 64)          # the eager window and the capture: host calls
    _quiet(eg)
    _quiet(ee)


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
def test_serial_trainer_ends_bitwise_equal_with_both_graphs(tmp_path):
    import plugin
    from synth_tensor_blob import SynthTensorBlob
    from synth_tensor_blob_inplace import SynthTensorBlobInplace
    from training.hip_trainer import TB, HipOffSerialTrainer, read_scalars

    N, S, K, iters, cap, warm = 8, 8, 8, 16, 64, 16
    finals, tars = [], []
    for graph in (False, True):
        folder = str(tmp_path / ("graph" if graph else "eager"))
        kw = _kw(BLOB, BLOB_A, BLOB_CT, buffer_max_size=cap, buffer_warm_size=warm, seed=3, sample_batch_size=S, sample_interval=K,
                 max_iteration=iters, log_save_interval=8, apprfunc_save_interval=100000, eval_interval=8, save_folder=folder,
                 ini_network_dir=None, hip_device_indices=True, reward_scale=0.25, sampler_name="hip_tensor_env_sampler",
                 evaluator_name="hip_tensor_env_evaluator", num_eval_episode=4, hip_obs_codebook=BOOK)
        torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
        env = SynthTensorBlobInplace if graph else SynthTensorBlob
        alg = plugin.create_alg(**kw)
        buf = plugin.create_buffer(**kw)
        e = alg.engine
        assert buf.engine is e and e.cnn_act
        smp = plugin.create_sampler(env=env(N, device="cuda", seed=4, frames="uint8"), **dict(kw, **(dict(hip_graph_sample=True) if graph else {})))
        ev = plugin.create_evaluator(eval_env=env(4, device="cuda", seed=6, frames="uint8"), **dict(kw, **(dict(hip_graph_eval=True) if graph else {})))
        assert ev.graph_eval == graph and smp.graph_sample == graph
        tr = plugin.create_trainer(alg, smp, buf, ev, **kw)
        assert type(tr) is HipOffSerialTrainer
        tr.train()
        e.sync()
        _quiet(e)
        n_samples = warm // S * S + (iters + K - 1) // K * S
        assert smp.get_total_sample_number() == n_samples and smp.act_step == n_samples // N
        logged = read_scalars(folder)[TB["tar_iter"]]
        assert len(logged["y"]) == 2                                    # evaluations at iterations 0 and 8: two windows of 16 each
        if graph:
            assert smp.graph_captures == 1 and smp.graph_replays == n_samples // S - 1 and e.act_counter_read() == smp.act_step
            assert ev.graph_captures == 1 and ev.graph_replays == 3     # eager window, capture (+ its replay), two replays
            assert e.debug_get("cnn_act_capture") == 1.0
        else:
            assert e.debug_get("cnn_act_capture") == 0.0
        tars.append([float(y) for y in logged["y"]])
        finals.append((e.buffer_digest(), buf.size, buf.ptr, e.online.cpu().clone(), e.target.cpu().clone(), e.adam_m.cpu().clone(),
                       e.adam_v.cpu().clone()))
    assert np.array_equal(_bits(np.array(tars[0])), _bits(np.array(tars[1]))) and np.isfinite(tars[0]).all()
    assert finals[0][:3] == finals[1][:3]
    for x, y in zip(finals[0][3:], finals[1][3:]):
        assert torch.equal(x, y)
