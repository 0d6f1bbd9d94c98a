"""CNN acting path (dsact_cnn_acting_enable): dsact_act_sample_batch / dsact_act_sample on image frames,
live and under a behaviour hold, against the torch module forward + the distribution's closed form; row independence across
the 64-frame chunks; unchanged refusals and unchanged stand-alone forward without / with the opt-in; the samplers' routes; and
the overlapped trainer on the whole stack against the same loop with nothing overlapped.

Shapes: (4, 84, 84) type_1 takes k_act_frames' generic quad form, (3, 96, 96) type_2 its RGB form.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle.dsact_oracle_cnn import cnn_config, synth_image_batch
from oracle.trainer_trajectory import TIME_TAGS, variant_case
from test_hip_cnn_parity import cnn_kwargs
from test_vec_acting import _check, _cpu_twin, _reference

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

SHAPES = [pytest.param((4, 84, 84), 2, "type_1", id="type_1"), pytest.param((3, 96, 96), 3, "type_2", id="type_2")]
LIM = 1.0
_cache = {}


def _kw(shape, A, ct, B=8, **over):
    return cnn_kwargs(shape, A, ct, B, hip_cnn_act=True, strict_rng=True, **over)


def _make(shape, A, ct, B=8, algorithm="DSAC_V2_HIP", seed=3, **over):
    torch.manual_seed(seed)
    mod = __import__(algorithm.lower())
    return getattr(mod, algorithm)(**_kw(shape, A, ct, B, algorithm=algorithm, **over))


def _shared(shape, A, ct):
    """(alg, CPU twin, frames[70], eps[70], the n = 70 call's results): built once per shape, never written afterwards"""
    key = (shape, A, ct)
    if key not in _cache:
        alg = _make(shape, A, ct)
        rng = np.random.default_rng(7)
        obs = rng.uniform(0.0, 1.0, (70,) + tuple(shape)).astype(np.float32)
        eps = rng.standard_normal((70, A)).astype(np.float32)
        a, lp = alg.engine.act_sample_batch(obs, eps)
        _cache[key] = (alg, _cpu_twin(alg, _kw(shape, A, ct)), obs, eps, (a.copy(), lp.copy()))
    return _cache[key]


@pytest.mark.parametrize("n", [1, 5, 64, 70])
@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_sample_equals_module_forward_and_reference_sample(shape, A, ct, n):
    alg, ref, obs, eps, _ = _shared(shape, A, ct)
    e = alg.engine
    assert e.cnn_act and e.debug_get("cnn_act") == 1.0 and e.debug_get("act_fast") == 1.0
    calls = e.debug_get("act_batch_calls")
    a, lp = e.act_sample_batch(obs[:n], eps[:n])
    assert a.shape == (n, A) and lp.shape == (n,)
    assert e.debug_get("act_batch_calls") - calls == -(-n // 64)   # chunks of 64 frames
    ra, rlp, rlg = _reference(ref, obs[:n], eps[:n])
    print("n=%d max |action - ref| = %.3g, max |logp - ref| = %.3g" % (n, np.abs(a - ra).max(), np.abs(lp - rlp).max()))
    _check(a, lp, ra, rlp, rlg, LIM, False, (ct, n))
    a_flat, lp_flat = e.act_sample_batch(obs[:n].reshape(n, -1), eps[:n])   # [n, O] rows are the same frames
    assert np.array_equal(a, a_flat) and np.array_equal(lp, lp_flat)
    if n == 5:   # device-resident inputs: the same rows by device address
        a2, lp2 = e.act_sample_batch(torch.from_numpy(obs[:n]).cuda(), torch.from_numpy(eps[:n]).cuda())
        assert np.array_equal(a, a2) and np.array_equal(lp, lp2)


@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_rows_do_not_depend_on_the_batch_or_the_chunk(shape, A, ct):
    alg, _, obs, eps, (a_all, lp_all) = _shared(shape, A, ct)
    for i in (0, 63, 64, 69):
        a, lp = alg.engine.act_sample_batch(obs[i:i + 1], eps[i:i + 1])
        assert np.array_equal(a[0], a_all[i]) and lp[0] == lp_all[i], i


@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_per_row_entry_point_is_the_batch_call_at_n1(shape, A, ct):
    alg, _, obs, eps, (a_all, lp_all) = _shared(shape, A, ct)
    a1, lp1 = alg.engine.act_sample(np.ascontiguousarray(obs[2]), np.ascontiguousarray(eps[2]))
    assert np.array_equal(a1, a_all[2]) and lp1[0] == lp_all[2]


@pytest.mark.parametrize("shape,A,ct", SHAPES)
def test_held_acting_is_the_policy_before_the_updates(shape, A, ct):
    B = 16
    alg = _make(shape, A, ct, B=B, policy_learning_rate=3e-3)
    e = alg.engine
    cfg = cnn_config(shape, A, ct)
    rng = np.random.default_rng(9)
    obs = rng.uniform(0.0, 1.0, (70,) + tuple(shape)).astype(np.float32)
    eps = rng.standard_normal((70, A)).astype(np.float32)
    r0 = e.act_sample_batch(obs, eps)
    holds, acts = e.debug_get("beh_holds"), e.debug_get("beh_acts")

    data = synth_image_batch(cfg, B, seed=20)
    e.behaviour_hold()
    assert e.debug_get("beh_held") == 1.0
    for it in range(4):
        torch.manual_seed(40 + it)
        alg.local_update(data, it)    # left unsynchronised
    held = e.act_sample_batch(obs, eps)
    assert np.array_equal(held[0], r0[0]) and np.array_equal(held[1], r0[1])
    a1, lp1 = e.act_sample(np.ascontiguousarray(obs[64]), np.ascontiguousarray(eps[64]))   # the per-row call is held too
    assert np.array_equal(a1, r0[0][64]) and lp1[0] == r0[1][64]
    e.behaviour_hold()            # a second hold replaces the snapshot: the policy behind the 4 updates
    held2 = e.act_sample_batch(obs, eps)
    e.behaviour_release()
    assert e.debug_get("beh_held") == 0.0
    e.sync()
    live = e.act_sample_batch(obs, eps)
    assert np.array_equal(held2[0], live[0]) and np.array_equal(held2[1], live[1])
    assert not np.array_equal(live[0], r0[0]), "the updates did not move the policy: the test shows nothing"
    assert e.debug_get("beh_holds") - holds == 2 and e.debug_get("beh_acts") - acts == 3
    assert e.debug_get("handoff_failures") == 0.0


def test_refusals_and_the_stand_alone_forward_are_unchanged():
    from dsact._ffi import DsactError
    from helpers import hip_kwargs

    shape, A, ct = (3, 96, 96), 3, "type_2"
    torch.manual_seed(3)
    from dsac_v2_hip import DSAC_V2_HIP

    alg = DSAC_V2_HIP(**cnn_kwargs(shape, A, ct, 8, strict_rng=True))   # no hip_cnn_act
    e = alg.engine
    assert not e.cnn_act and e.debug_get("cnn_act") == 0.0 and e.debug_get("act_fast") == 0.0
    rng = np.random.default_rng(1)
    obs = rng.uniform(0.0, 1.0, (5,) + shape).astype(np.float32)
    eps = rng.standard_normal((5, A)).astype(np.float32)
    with pytest.raises(DsactError, match="E_INVALID"):
        e.act_sample_batch(obs, eps)
    with pytest.raises(DsactError, match="E_INVALID"):
        e.act_sample(np.ascontiguousarray(obs[0]), np.ascontiguousarray(eps[0]))
    with pytest.raises(DsactError, match="E_INVALID"):
        e.behaviour_hold()
    fwd0, mode0 = e.policy_forward(obs).copy(), e.act_mode_batch(obs).copy()
    e.enable_cnn_acting()
    e.enable_cnn_acting()         # idempotent
    assert e.cnn_act and e.debug_get("cnn_act") == 1.0
    a, lp = e.act_sample_batch(obs, eps)
    assert np.isfinite(a).all() and np.isfinite(lp).all()
    np.testing.assert_array_equal(e.policy_forward(obs), fwd0)
    np.testing.assert_array_equal(e.act_mode_batch(obs), mode0)
    # the same weights enabled at construction act bit for bit like the handle enabled later
    b, lpb = _make(shape, A, ct).engine.act_sample_batch(obs, eps)
    assert np.array_equal(a, b) and np.array_equal(lp, lpb)

    torch.manual_seed(0)
    mlp = DSAC_V2_HIP(**hip_kwargs(16, 4, (64, 64), 64, hip_cnn_act=True))   # the kwarg does nothing with MLP nets
    assert not mlp.engine.cnn_act
    with pytest.raises(DsactError, match="E_INVALID"):
        mlp.engine.enable_cnn_acting()
    assert not mlp.engine.cnn_act and mlp.engine.debug_get("cnn_act") == 0.0


def test_dsac_v1_cnn_handle():
    shape, A, ct = (3, 96, 96), 3, "type_2"
    alg = _make(shape, A, ct, algorithm="DSAC_V1_HIP", TD_bound=10.0)
    ref = _cpu_twin(alg, _kw(shape, A, ct, algorithm="DSAC_V1_HIP", TD_bound=10.0), module="dsac_v1_hip")
    rng = np.random.default_rng(4)
    obs = rng.uniform(0.0, 1.0, (5,) + shape).astype(np.float32)
    eps = rng.standard_normal((5, A)).astype(np.float32)
    a, lp = alg.engine.act_sample_batch(obs, eps)
    _check(a, lp, *_reference(ref, obs, eps), LIM, False, "v1")


def test_samplers_take_the_cnn_acting_path():
    import plugin

    shape, A = (3, 96, 96), 3
    kw = _kw(shape, A, "type_2", env_id="synth_blob", sample_batch_size=8, seed=4)
    torch.manual_seed(0)
    alg = plugin.create_alg(**kw)
    e = alg.engine
    smp = plugin.create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=4, **kw)
    smp.networks = alg.networks
    assert smp.route() == "gpu"
    torch.manual_seed(6)
    batch, _ = smp.sample()
    O = int(np.prod(shape))
    assert len(batch) == 8 and batch.packed[0].shape == (8, O) and batch.packed[3].shape == (8, O)
    assert batch.packed[1].shape == (8, A) and batch.packed[5].shape == (8,)
    torch.manual_seed(6)
    a, lp = e.act_sample_batch(batch.packed[0][:4], torch.randn(4, A))
    np.testing.assert_array_equal(batch.packed[1][:4], a)
    np.testing.assert_array_equal(batch.packed[5][:4], lp)

    one = plugin.create_sampler(**kw)   # HipOffSampler
    one.networks = alg.networks
    assert one.per_row_engine() is e
    calls = e.debug_get("act_batch_calls")
    torch.manual_seed(6)
    b1, _ = one.sample()
    assert e.debug_get("act_batch_calls") - calls == 8 and b1.packed[0].shape == (8, O)
    torch.manual_seed(6)
    a0, lp0 = e.act_sample_batch(b1.packed[0][:1], torch.randn(1, A))   # one torch.randn(1, A) per step, as the general path
    np.testing.assert_array_equal(b1.packed[1][0], a0[0])
    # without the kwarg on the sampler's side the routes are today's
    kw0 = dict(kw, hip_cnn_act=False)
    off = plugin.create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=4, **kw0)
    off.networks = alg.networks
    assert off.route() == "module"


# ---- the overlapped trainer, the whole stack ----------------------------------------------------------------------------------
RAM_TAG = "RAM/RAM [MB]-RL iter"
VEC = dict(sampler_name="hip_vec_off_sampler", vector_env_num=4)


def _run(tmp, name, trainer, sync_first=False, **sampler):
    """one training run of the cnn_si8 case on the HIP stack, recorded by run_loop; sync_first: every sampler call first waits
    for the engine's stream, so nothing overlaps"""
    import plugin
    from test_async_trainer_host import run_loop
    from test_trainer_trajectory import derived_kwargs

    case = dict(variant_case("cnn_si8"), algorithm="DSAC_V2_HIP", buffer_name="hip_replay_buffer", hip_cnn_act=True, trainer=trainer,
                **sampler)
    kw = derived_kwargs(case, str(tmp / name), strict_rng=True)
    alg = plugin.create_alg(**kw)
    buffer = plugin.create_buffer(**kw)
    assert buffer.engine is alg.engine and alg.engine.cnn_act

    def make(alg_, smp, buf, ev, **k):
        if sync_first:
            inner = smp.sample
            smp.sample = lambda: (alg_.engine.sync(), inner())[1]
        return plugin.create_trainer(alg_, smp, buf, ev, **k)

    got, tr = run_loop(kw, make, alg=alg, buffer=buffer)
    e = alg.engine
    e.sync()
    got["ring"] = (int(e.buffer_size), tuple(e.buffer_digest()))
    got["beh"] = {k: e.debug_get(k) for k in ("beh_holds", "beh_acts", "beh_held", "handoff_failures")}
    return got, tr, case


def _exactly_equal(x, y):
    if any(x[k] != y[k] for k in ("indices", "buffer", "saved", "evals", "tb", "warm", "apprfunc_dir", "samples", "ring")):
        return False
    if len(x["adds"]) != len(y["adds"]) or not all(np.array_equal(a, b) for a, b in zip(x["adds"], y["adds"])):
        return False
    wall = "Evaluation/2. TAR-Total time [s]"
    if len(x["scalars"]) != len(y["scalars"]):
        return False
    for g, w in zip(x["scalars"], y["scalars"]):
        if g[0] != w[0] or not (g[0] == wall or g[1] == w[1]):
            return False
        if g[0] not in TIME_TAGS and g[0] != RAM_TAG and g[2] != w[2]:
            return False
    return True


def _close_at_the_async_gates(got, want):
    """the gates of tests/test_async_trainer_gpu.py (for an update that is not run-to-run deterministic at this shape)"""
    for k in ("indices", "buffer", "saved", "apprfunc_dir", "warm", "samples"):
        assert got[k] == want[k], k
    assert [t[:2] for t in got["tb"]] == [t[:2] for t in want["tb"]]
    for g, w in zip(got["tb"], want["tb"]):
        for k, (a, b) in enumerate(zip(g[2:], w[2:])):
            assert abs(a - b) <= (1e-6 + 1e-5 * abs(b) if k == 7 else 1e-4), (g[:2], k, a, b)
    for (i0, a), (i1, b) in zip(got["evals"], want["evals"]):
        assert i0 == i1 and abs(a - b) <= 1e-4 * abs(b), (i0, a, b)


@pytest.mark.parametrize("sampler", ["single", "vec"])
def test_overlapped_trainer_computes_what_the_unoverlapped_loop_computes(tmp_path, sampler):
    from training.hip_async_trainer import HipOffAsyncTrainer

    smp = VEC if sampler == "vec" else {}
    b1, _, _ = _run(tmp_path, "b1", "hip_off_async_trainer", sync_first=True, **smp)
    b2, _, _ = _run(tmp_path, "b2", "hip_off_async_trainer", sync_first=True, **smp)
    deterministic = _exactly_equal(b1, b2)       # precondition: the update is run-to-run deterministic at this shape
    print("two unoverlapped runs bitwise equal:", deterministic)
    a, tr, case = _run(tmp_path, "a", "hip_off_async_trainer", **smp)
    assert type(tr) is HipOffAsyncTrainer
    if sampler == "vec":
        assert tr.sampler.route() == "gpu"
    else:
        assert tr.sampler.per_row_engine() is tr.alg.engine
    if deterministic:
        assert _exactly_equal(a, b1), "overlap changed what the loop computes"
    else:
        _close_at_the_async_gates(a, b1)
    K = case["sample_interval"]
    assert a["beh"]["beh_holds"] == -(-case["max_iteration"] // K)
    assert a["beh"]["beh_acts"] > 0 and a["beh"]["beh_held"] == 0.0 and a["beh"]["handoff_failures"] == 0.0
    # the lag is real: S_0 is the serial trainer's, S_1 was collected with a policy one group old
    serial, _, _ = _run(tmp_path, "serial", "off_serial_trainer", **smp)
    assert serial["warm"] == a["warm"] and len(serial["adds"]) == len(a["adds"])
    for i in range(a["warm"] + 1):
        np.testing.assert_array_equal(a["adds"][i], serial["adds"][i])
    s1 = a["warm"] + 1
    assert not np.array_equal(a["adds"][s1], serial["adds"][s1])
