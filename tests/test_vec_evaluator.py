"""dsact_act_mode_batch (the evaluator's deterministic acting, csrc/dsact_act_batch.h kMode) and HipVecEvaluator on the GPU:
both routes against the torch module forward + dist.mode(), row independence, the mode against the sample with eps = 0,
live weights behind unsynchronised updates, and a trainer run with the vectorised evaluator against HipEvaluator."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs
from test_acting_live_weights import (GUARD, _batch, _fill_ring, _fp64_policy, _kw, _live_policy, _make, _policy_out_bias,
                                      _within)
from test_hip_parity import make_pair
from test_vec_acting import MATRIX, _cpu_twin

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

HOST_ALL, GPU_ALL = 10 ** 6, 0   # debug switch "mode_host_rows": every row count on the host route / on the GPU route


def _module_mode(ref, obs):
    with torch.no_grad():
        return ref.create_action_distributions(ref.policy(torch.from_numpy(obs))).mode().numpy().reshape(obs.shape[0], -1)


def _route(e, route):
    e.debug_set("mode_host_rows", HOST_ALL if route == "host" else GPU_ALL)


def _mode(e, obs, route):
    """act_mode_batch on the named route; asserts that the route was taken"""
    _route(e, route)
    calls = e.debug_get("act_mode_calls")
    a = e.act_mode_batch(obs)
    assert (e.debug_get("act_mode_calls") > calls) == (route == "gpu"), route
    return a


@pytest.mark.parametrize("O,A,hid,B,lim,over", MATRIX)
def test_mode_batch_equals_module_mode_on_both_routes(O, A, hid, B, lim, over):
    alg, _ = make_pair(O, A, hid, B, act_limit=lim, seed=61, **over)
    e = alg.engine
    ref = _cpu_twin(alg, hip_kwargs(O, A, hid, B, act_limit=lim, **over))
    rng = np.random.default_rng(3)
    routes = ("host", "gpu") if e.debug_get("act_host") == 1.0 else ("gpu",)
    for n in (1, 7, 64, 300):
        obs = (3.0 * rng.standard_normal((n, O))).astype(np.float32)
        want = _module_mode(ref, obs)
        for route in routes:
            a = _mode(e, obs, route)
            assert a.shape == (n, A) and a.dtype == np.float32
            np.testing.assert_allclose(a, want, rtol=1e-5, atol=1e-5, err_msg=str((route, n, O, A, hid, over)))
            assert np.all(a <= lim) and np.all(a >= -lim)
        if n == 7:   # device-resident rows: the same actions by device address
            assert np.array_equal(e.act_mode_batch(torch.from_numpy(obs).cuda()), a)


def test_dsac_v1_handle():
    from test_hip_v1_parity import make_pair as make_v1

    O, A, hid, B = 24, 6, (64, 64), 64
    alg, _ = make_v1(O, A, hid, B, seed=5)
    ref = _cpu_twin(alg, hip_kwargs(O, A, hid, B, algorithm="DSAC_V1_HIP", TD_bound=10.0), module="dsac_v1_hip")
    obs = np.random.default_rng(4).standard_normal((33, O)).astype(np.float32)
    want = _module_mode(ref, obs)
    for route in ("host", "gpu"):
        np.testing.assert_allclose(_mode(alg.engine, obs, route), want, rtol=1e-5, atol=1e-5, err_msg=route)


@pytest.mark.parametrize("shape,A,conv_type", [((4, 84, 84), 2, "type_1"), ((3, 96, 96), 3, "type_2")])
def test_cnn_mode_batch_equals_module_mode(shape, A, conv_type):
    import plugin
    from test_hip_cnn_parity import cnn_kwargs

    kw = cnn_kwargs(shape, A, conv_type, 8, seed=4, strict_rng=False)
    torch.manual_seed(0)
    alg = plugin.create_alg(**kw)
    ref = _cpu_twin(alg, kw)
    rng = np.random.default_rng(8)
    for n in (1, 5, 70):   # 70: two chunks of the stand-alone forward
        obs = rng.uniform(0, 1, (n,) + shape).astype(np.float32)
        a = alg.engine.act_mode_batch(obs)
        np.testing.assert_allclose(a, _module_mode(ref, obs), rtol=1e-5, atol=1e-5, err_msg=str((conv_type, n)))
    ev = plugin.create_evaluator(hip_eval_env_num=2, eval_envs=[object(), object()], networks=alg.networks)
    assert ev.route() == "engine"


def test_refusals():
    from dsact._ffi import DsactError
    from dsact.engine import DsactEngine

    e = DsactEngine(8, 3, (64, 64), 32)
    with pytest.raises(DsactError):          # no action limits
        e.act_mode_batch(np.zeros((2, 8), np.float32))
    e.close()
    from dsac_v2_hip import ApproxContainer

    torch.manual_seed(0)                     # an unattached container: the module forward
    ev = __import__("plugin").create_evaluator(hip_eval_env_num=2, eval_envs=[object(), object()],
                                               networks=ApproxContainer(**hip_kwargs(8, 3, (64, 64), 32)))
    assert ev.route() == "module"


def test_gpu_rows_do_not_depend_on_the_batch():
    alg, _ = make_pair(376, 17, (256, 256, 256), 256, seed=7)
    e = alg.engine
    obs = np.random.default_rng(6).standard_normal((1100, 376)).astype(np.float32)
    full = _mode(e, obs, "gpu")
    for n in (1, 33):
        assert np.array_equal(_mode(e, obs[:n], "gpu"), full[:n]), n
    perm = np.random.default_rng(7).permutation(1100)
    assert np.array_equal(_mode(e, obs[perm], "gpu"), full[perm])
    for i in (0, 31, 32, 517, 1024, 1099):
        assert np.array_equal(_mode(e, obs[i:i + 1], "gpu"), full[i:i + 1]), i


@pytest.mark.parametrize("O,A,hid,B,lim,over", [m for m in MATRIX if "policy_act_distribution" not in m[5]])
def test_tanh_mode_equals_sample_with_zero_eps(O, A, hid, B, lim, over):
    alg, _ = make_pair(O, A, hid, B, act_limit=lim, seed=62, **over)
    e = alg.engine
    obs = (2.0 * np.random.default_rng(9).standard_normal((300, O))).astype(np.float32)
    zeros = np.zeros((300, A), np.float32)
    a, _ = e.act_sample_batch(obs, zeros)
    assert np.array_equal(_mode(e, obs, "gpu"), a)
    if e.debug_get("act_host") == 1.0:   # the host route: the host forward's sample with eps = 0, row by row
        got = _mode(e, obs[:8], "host")
        for i in range(8):
            a1, _ = e.act_sample(obs[i], zeros[i])
            assert np.array_equal(got[i], a1), i


def test_host_route_matches_gpu_route():
    alg, _ = make_pair(376, 17, (256, 256, 256), 256, seed=11)
    e = alg.engine
    assert e.debug_get("act_host") == 1.0
    obs = np.random.default_rng(12).standard_normal((64, 376)).astype(np.float32)
    np.testing.assert_allclose(_mode(e, obs, "host"), _mode(e, obs, "gpu"), rtol=1e-5, atol=1e-5)
    e.debug_set("mode_host_rows", 16)
    assert e.debug_get("mode_host_rows") == 16.0


# ---- live weights: every acting route right after each update path -------------------------------------------------
class ModeActing:
    """both routes of dsact_act_mode_batch right after an event, against the fp64 forward of the arena's weights
    (tests/test_acting_live_weights.py: its mode is the tanh-Gauss action at eps = 0)"""

    def __init__(self, alg, kw, rows=1100, seed=3):
        self.alg, self.kw, self.e = alg, kw, alg.engine
        assert self.e.debug_get("act_host") == 1.0
        rng = np.random.default_rng(seed)
        self.obs = rng.standard_normal((rows, self.e.obs_dim)).astype(np.float32)
        self.zeros = np.zeros((rows, self.e.act_dim), np.float32)
        self.ref = None
        self.check("initial")

    def check(self, tag, torch_write=False):
        e, obs = self.e, self.obs
        if torch_write:   # the evaluator's noticing point (HipVecEvaluator.run_evaluation)
            e.note_torch_writes(self.alg.networks.policy.parameters())
        got = {}
        for route, ns in (("host", (1, 33)), ("gpu", (1, 33, len(obs)))):   # the host route first: nothing has synchronised yet
            for n in ns:
                got["%s n=%d" % (route, n)] = (n, _mode(e, obs[:n], route))
        ref = _fp64_policy(_live_policy(self.alg, self.kw), obs, self.zeros)
        for k, (n, a) in got.items():
            _within(a, ref["a"][:n], ref["da"][:n], "%s / %s mode" % (tag, k))
        if self.ref is not None:
            r = float(np.max(np.abs(ref["a"][:1] - self.ref["a"][:1]) / ref["da"][:1]))
            assert r >= GUARD, "%s: ill-posed -- the previous weights' actions are only %.3g bounds away" % (tag, r)
        self.ref = ref


@pytest.mark.parametrize("O,A,hid,B,lim", [pytest.param(376, 17, (256, 256, 256), 256, 0.4, id="humanoid"),
                                           pytest.param(5, 1, (33,), 16, 2.0, id="ragged")])
def test_mode_acts_on_the_live_weights(O, A, hid, B, lim):
    from dsac_v2_hip import HipBatchGroup

    kw = _kw(O, A, hid, B, lim, seed=5)
    alg = _make(kw, 4)
    e = alg.engine
    rows = _fill_ring(e, 1024)
    ac = ModeActing(alg, kw)
    alg.local_update(_batch(np.random.default_rng(2), B, O, A, lim), 0)
    ac.check("local_update")
    e.gather(rows[1]); e.step(2)
    ac.check("eager step")
    e.gather(rows[2]); e.compute_grads(4); e.apply_update(4)
    ac.check("compute_grads + apply_update")
    alg2 = _make(kw, 9)
    _, info = alg2.get_remote_update_info(_batch(np.random.default_rng(7), B, O, A, lim), 6)
    alg.remote_update(info)
    ac.check("remote_update")
    del info, alg2
    alg.local_update_group(HipBatchGroup(e, rows[:4]), 8)
    ac.check("local_update_group")
    e.run_group(12, rows[:4])
    ac.check("run_group")
    e.graph_build(4)
    e.graph_run(16, 8)
    ac.check("graph_run")
    sd = {k: v.clone() for k, v in alg.networks.state_dict().items()}
    for k in sd:
        if k.startswith("policy.policy.") and k.endswith("bias"):
            sd[k] += 0.05
    alg.networks.load_state_dict(sd)
    ac.check("load_state_dict")
    p = _policy_out_bias(alg)
    with torch.no_grad():
        p.add_(0.05)
    torch.cuda.synchronize()
    ac.check("in-place p.add_ under no_grad", torch_write=True)
    p.data.copy_(p.data + 0.06)
    torch.cuda.synchronize()
    e.policy_dirty()
    ac.check("p.data.copy_ + policy_dirty()")


def test_mode_after_dp_steps():
    import torch.distributed as dist

    from test_acting_live_weights import DP, _dp_handle, _updater

    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29548")
        dist.init_process_group("gloo", rank=0, world_size=1)
        created = True
    try:
        alg, kw = _dp_handle()
        e = alg.engine
        dp = _updater(e)
        ac = ModeActing(alg, kw)
        e.dp_begin(0)
        dp.step()
        ac.check("dp eager step")
        alg2, kw2 = _dp_handle(seed=6)
        dp2 = _updater(alg2.engine, native=True)
        ac2 = ModeActing(alg2, kw2)
        assert dp2.build_graph(2, fallback=False)
        dp2.run_graph(0, 4)
        ac2.check("dp graph_run")
        alg2.engine.comm_destroy()
        assert DP[1] == e.act_dim
    finally:
        if created:
            dist.destroy_process_group()


# ---- the trainer with the vectorised evaluator ---------------------------------------------------------------------
def _train(tmp_path, vec, route=None):
    import plugin
    from training.hip_trainer import HipEvaluator

    N, E = 3, 4
    kw = hip_kwargs(376, 17, (256, 256, 256), 256, env_id="synth_humanoid", sample_batch_size=20, buffer_warm_size=256,
                    buffer_max_size=10000, max_iteration=21, log_save_interval=1000, apprfunc_save_interval=10000,
                    eval_interval=10, num_eval_episode=E, ini_network_dir=None, save_folder=str(tmp_path), seed=3,
                    sample_interval=1)
    if vec:
        kw["hip_eval_env_num"] = N
    torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
    alg = plugin.create_alg(**kw)
    if route is not None:
        _route(alg.engine, route)
    sampler = plugin.create_sampler(**kw)
    buf = plugin.create_buffer(**kw)
    ev = plugin.create_evaluator(**kw)
    assert type(ev).__name__ == ("HipVecEvaluator" if vec else "HipEvaluator")
    records = []
    if vec:
        orig = ev.run_evaluation

        def rec(it):
            envs = copy.deepcopy(ev.envs)      # the environments as this evaluation finds them
            calls = alg.engine.debug_get("act_mode_calls")
            tar = orig(it)
            assert ev.route() == "engine" and (alg.engine.debug_get("act_mode_calls") > calls) == (route == "gpu")
            rets = [None] * E
            for i, env in enumerate(envs):   # HipEvaluator on each environment's copy, given its episodes
                one = HipEvaluator(eval_env=env, networks=alg.networks, num_eval_episode=1)
                for ep in range(i, E, N):
                    rets[ep] = one.run_an_episode()
            records.append((tar, list(ev.returns), rets, ev.steps))
            return tar

        ev.run_evaluation = rec
    tr = plugin.create_trainer(alg, sampler, buf, ev, **kw)
    tr.train()
    e = alg.engine
    e.sync()
    state = [t.detach().cpu().numpy().copy() for t in (e.online, e.target, e.adam_m, e.adam_v)]
    return state, e.get_state(), records


@pytest.mark.parametrize("route", ["host", "gpu"])
def test_trainer_with_vec_evaluator_matches_hip_evaluator(route, tmp_path):
    base, base_st, _ = _train(tmp_path / "base", vec=False)
    got, got_st, records = _train(tmp_path / "vec", vec=True, route=route)
    for a, b in zip(got, base):
        assert np.array_equal(a, b)
    assert got_st == base_st
    assert len(records) == 3   # iterations 0, 10, 20
    A, lim, delta = 17, 0.4, 1e-5
    for tar, rets, ref, steps in records:
        assert steps == 2000   # 4 episodes of 1000 steps over 3 environments
        # reward -|a|^2 per step: an action within delta of the reference's moves it by <= A (2 lim delta + delta^2)
        bound = 1000 * A * (2 * lim * delta + delta * delta)
        for r, q in zip(rets, ref):
            assert abs(r - q) <= bound, (r, q, bound)
        assert abs(tar - np.mean(ref)) <= bound
