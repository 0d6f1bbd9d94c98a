"""Held behaviour policy (dsact_behaviour_hold): the overlapped trainer's acting.

Hold, enqueue a group of 64 updates, then act. The held calls -- dsact_act_sample on the host route and on a handle without
host acting (hip_host_act=False: the batched forward at n = 1 on the acting stream), dsact_act_sample_batch at N = 1, 16,
64, 256 -- must return, bit for bit, what a second engine loaded with the weights from before the group returns acting live
through the same kernels, and must not wait for the group (the handle's stream is still busy when they return).
dsact_act_mode_batch and dsact_policy_forward stay live under a hold; after the release every route is live again.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch

from helpers import hip_kwargs

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

GROUP = 64
SHAPES = [
    pytest.param("DSAC_V2_HIP", 376, 17, (256, 256, 256), 256, 0.4, id="humanoid"),     # the BASELINE policy
    pytest.param("DSAC_V2_HIP", 5, 1, (33,), 16, 2.0, id="padded"),                    # stored zero-padded to 64 wide
    pytest.param("DSAC_V1_HIP", 16, 4, (64, 64), 64, 0.3, id="v1"),
]


def _make(algorithm, O, A, hid, B, lim, host_act, seed=4):
    kw = hip_kwargs(O, A, hid, B, act_limit=lim, algorithm=algorithm, seed=5, hip_pad_widths=True, policy_learning_rate=3e-3,
                    hip_host_act=host_act)
    torch.manual_seed(seed)
    mod = __import__(algorithm.lower())
    return getattr(mod, algorithm)(**kw)


def _fill_ring(e, N=1024, seed=1):
    e.buffer_create(N)
    g = torch.Generator(device="cuda").manual_seed(seed)
    O, A = e.obs_dim, e.act_dim
    e.buffer_fill_device(0, torch.randn(N, O, device="cuda", generator=g), torch.rand(N, A, device="cuda", generator=g) - .5,
                         torch.randn(N, device="cuda", generator=g), torch.randn(N, O, device="cuda", generator=g),
                         (torch.rand(N, device="cuda", generator=g) < .05).float())
    return np.random.default_rng(seed).integers(0, N, size=(GROUP, e.batch))


def _load(dst, src):
    """dst's arenas := src's (both engines idle afterwards); the acting snapshots of dst are stale from here on"""
    src.sync()
    dst.sync()
    with torch.no_grad():
        for k in ("online", "target"):
            getattr(dst, k).copy_(getattr(src, k))
    torch.cuda.synchronize()
    dst.policy_dirty()


def _act1(e, obs, eps, host_act):
    """one transition's acting as the sampler does it: dsact_act_sample (reference for hip_host_act=False under a hold: the
    batched forward at n = 1, live)"""
    a, lp = e.act_sample(obs, eps)
    return a.copy(), lp.copy()


@pytest.mark.parametrize("host_act", [True, False], ids=["host", "gpu"])
@pytest.mark.parametrize("algorithm,O,A,hid,B,lim", SHAPES)
def test_held_acting_is_the_policy_before_the_group(algorithm, O, A, hid, B, lim, host_act):
    alg = _make(algorithm, O, A, hid, B, lim, host_act)
    e = alg.engine
    rows = _fill_ring(e)
    e.run_group(0, rows)            # (captures the group's graph: the held run below is a replay)
    ref = _make(algorithm, O, A, hid, B, lim, host_act, seed=11)
    _load(ref.engine, e)            # theta_before
    assert e.debug_get("act_host") == (1.0 if host_act else 0.0)
    rng = np.random.default_rng(3)
    obs1 = rng.standard_normal(O).astype(np.float32)
    eps1 = rng.standard_normal(A).astype(np.float32)
    batches = {n: (rng.standard_normal((n, O)).astype(np.float32), rng.standard_normal((n, A)).astype(np.float32))
               for n in (1, 16, 64, 256)}

    alg.hold_behaviour()
    assert e.debug_get("beh_held") == 1.0
    e.run_group(GROUP, rows)        # 64 updates enqueued behind the hold
    t0 = time.perf_counter()
    a1, lp1 = _act1(e, obs1, eps1, host_act)
    busy_after_sample = not e.stream_idle()
    t1 = time.perf_counter()
    held_batch = {1: e.act_sample_batch(*batches[1])}
    busy_after_batch = not e.stream_idle()
    t2 = time.perf_counter()
    for n, (o, x) in batches.items():
        if n > 1:
            held_batch[n] = e.act_sample_batch(o, x)
    took = "act_sample %.0f us, act_sample_batch(1) %.0f us" % (1e6 * (t1 - t0), 1e6 * (t2 - t1))
    assert busy_after_sample, "the held dsact_act_sample waited for the group (%s)" % took
    assert busy_after_batch, "the held dsact_act_sample_batch waited for the group (%s)" % took
    assert e.debug_get("beh_acts") == 1 + len(batches)

    # theta_before acting live through the same kernels
    if host_act:
        ra1, rlp1 = _act1(ref.engine, obs1, eps1, host_act)
    else:
        ra, rlp = ref.engine.act_sample_batch(obs1[None], eps1[None])
        ra1, rlp1 = ra[0], rlp[:1]
    np.testing.assert_array_equal(a1, ra1)
    np.testing.assert_array_equal(lp1, rlp1)
    for n, (o, x) in batches.items():
        ra, rlp = ref.engine.act_sample_batch(o, x)
        np.testing.assert_array_equal(held_batch[n][0], ra, err_msg="N=%d" % n)
        np.testing.assert_array_equal(held_batch[n][1], rlp, err_msg="N=%d" % n)

    # act_mode_batch / policy_forward under the hold: the live weights after the group
    e.sync()
    mode_held = e.act_mode_batch(batches[64][0])
    fwd_held = e.policy_forward(obs1)
    before_mode = ref.engine.act_mode_batch(batches[64][0])
    _load(ref.engine, e)            # theta_after
    np.testing.assert_array_equal(mode_held, ref.engine.act_mode_batch(batches[64][0]))
    np.testing.assert_array_equal(fwd_held, ref.engine.policy_forward(obs1))
    assert not np.array_equal(mode_held, before_mode), "the group did not move the policy: the test shows nothing"
    # a held call after the group completed still acts with theta_before
    np.testing.assert_array_equal(e.act_sample_batch(*batches[16])[0], held_batch[16][0])

    # release: live again
    alg.release_behaviour()
    assert e.debug_get("beh_held") == 0.0
    a2, lp2 = _act1(e, obs1, eps1, host_act)
    ra2, rlp2 = _act1(ref.engine, obs1, eps1, host_act)
    np.testing.assert_array_equal(a2, ra2)
    np.testing.assert_array_equal(lp2, rlp2)
    assert not np.array_equal(a2, a1)
    for n in (1, 256):
        got, want = e.act_sample_batch(*batches[n]), ref.engine.act_sample_batch(*batches[n])
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])

    # a second hold replaces the snapshot (theta_after now), whatever is enqueued behind it
    alg.hold_behaviour()
    e.run_group(2 * GROUP, rows)
    got = e.act_sample_batch(*batches[64])
    want = ref.engine.act_sample_batch(*batches[64])
    np.testing.assert_array_equal(got[0], want[0])
    alg.release_behaviour()
    e.sync()


def test_hold_is_refused_under_capture_and_on_cnn_handles():
    from dsact._ffi import DsactError
    from dsact.engine import DsactEngine
    from oracle.dsact_oracle_cnn import cnn_config

    alg = _make("DSAC_V2_HIP", 16, 4, (64, 64), 64, 0.3, True)
    e = alg.engine
    e.sync()
    g = torch.cuda.CUDAGraph()
    refused = None
    with torch.cuda.graph(g, stream=e.torch_stream, capture_error_mode="relaxed"):
        try:
            e.behaviour_hold()
        except DsactError as ex:
            refused = str(ex)
    del g
    assert refused is not None and "E_STATE" in refused and "capture" in refused, refused
    assert e.debug_get("beh_held") == 0.0
    e.behaviour_hold()            # outside a capture: accepted
    e.behaviour_release()
    e.sync()

    cfg = cnn_config((3, 96, 96), 3, "type_2")
    c = DsactEngine(cfg["obs_dim"], 3, list(cfg["hidden"]), 16, conv_type="type_2")
    with pytest.raises(DsactError, match="E_INVALID"):
        c.behaviour_hold()
    c.close()
