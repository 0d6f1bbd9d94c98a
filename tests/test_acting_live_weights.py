"""Every acting route acts with the policy weights that are in the arena NOW, right after every path that moves them.

The host-side acting path (csrc/dsact_host_act.h) reads a pinned snapshot of the policy that is only as fresh as the last
path that bumped `pol_epoch` or enqueued a copy behind its update. A path that forgets fails nothing by itself: the sampler
just acts with old weights. So each case here

  * takes an fp64 forward of the live weights (an unattached CPU container loaded from `networks.state_dict()` after
    `engine.sync()`) as the reference, with a per-output bound derived from fp32 accumulation (`_fp64_policy`);
  * calls every acting route right behind the weight-moving event -- no `debug_set("host_act")` and no `policy_dirty()` in
    between: host `act_sample`, host `policy_forward(n = 1)`, the module forward at n = 1, `act_sample_batch` at n = 1, 33
    (crosses a 32-row tile) and 1,100 (crosses the 1,024-row chunk), the module forward at n = 40, and last the one-launch
    GPU forward (`host_act` = 0, selected only after the host results were taken);
  * asserts the separation guard: the fp64 forward of the PREVIOUS weights is at least 10 bounds away from the live one,
    so a stale snapshot cannot pass.

Torch writes the engine cannot see through a version counter (`p.data.copy_`, a collective on the arena) follow the
contract of INTEGRATION.md section 1: the caller (or DataParallelUpdater) calls `engine.policy_dirty()`.
"""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

U = 2.0 ** -24            # fp32 unit roundoff
SAFETY = 2.0              # on top of the first-order bound: the fp32 rounding of the stored intermediates
PROPAGATE = 1.0          # incoming error bounds through a layer: this many times their root-sum-square
GUARD = 10.0              # live vs previous weights: at least this many bounds apart
LOG_EPS = 1e-6            # dsac_v2_hip._LOG_EPS
SKIP_ACTOR = 1            # DSACT_F_SKIP_ACTOR_ON_OFF_ITERS
N_ROWS = 1100


def _kw(O, A, hid, B, lim, **over):
    """the plugin's defaults (hip_pad_widths=True) with a policy learning rate large enough that one update moves the
    logits by many fp32 bounds"""
    over.setdefault("hip_pad_widths", True)
    over.setdefault("policy_learning_rate", 3e-3)
    return hip_kwargs(O, A, hid, B, act_limit=lim, **over)


def _make(kw, seed):
    torch.manual_seed(seed)
    if kw["algorithm"] == "DSAC_V1_HIP":
        from dsac_v1_hip import DSAC_V1_HIP
        return DSAC_V1_HIP(**kw)
    from dsac_v2_hip import DSAC_V2_HIP
    return DSAC_V2_HIP(**kw)


def _fill_ring(e, N, seed=1):
    e.buffer_create(N)
    g = torch.Generator(device="cuda").manual_seed(seed)
    O, A = e.obs_dim, e.act_dim
    e.buffer_fill_device(0, torch.randn(N, O, device="cuda", generator=g), torch.rand(N, A, device="cuda", generator=g) - .5,
                         torch.randn(N, device="cuda", generator=g), torch.randn(N, O, device="cuda", generator=g),
                         (torch.rand(N, device="cuda", generator=g) < .05).float())
    rows = np.random.default_rng(seed).integers(0, N, size=(16, e.batch))
    e.upload_index_table(rows)
    return rows


def _batch(rng, B, O, A, lim):
    return {"obs": torch.from_numpy(rng.standard_normal((B, O)).astype(np.float32)),
            "act": torch.from_numpy(rng.uniform(-lim, lim, (B, A)).astype(np.float32)),
            "rew": torch.from_numpy(rng.standard_normal(B).astype(np.float32)),
            "obs2": torch.from_numpy(rng.standard_normal((B, O)).astype(np.float32)),
            "done": torch.zeros(B)}


def _live_policy(alg, kw):
    """[(W, b, activation)] float64 of the policy in the arena now, through an unattached CPU container (tests/test_vec_acting.py
    _cpu_twin), plus its log-std clamp and action limits"""
    alg.engine.sync()
    ref = __import__("dsac_v1_hip" if kw["algorithm"] == "DSAC_V1_HIP" else "dsac_v2_hip").ApproxContainer(**kw)
    ref.load_state_dict({k: v.detach().cpu() for k, v in alg.networks.state_dict().items()})
    ref = ref.double()
    pol = ref.policy
    assert pol.std_type == "mlp_shared"
    mods = list(pol.policy)
    layers = []
    for lin, act in zip(mods[0::2], mods[1::2]):
        name = type(act).__name__
        assert name in ("GELU", "Identity"), name
        layers.append((lin.weight.detach().numpy(), lin.bias.detach().numpy(), name))
    hi, lo = pol.act_high_lim.numpy(), pol.act_low_lim.numpy()
    return {"layers": layers, "ls": (pol.min_log_std, pol.max_log_std), "half": (hi - lo) / 2, "center": (hi + lo) / 2}


def _fp64_policy(P, obs, eps):
    """logits (mean | std), tanh-Gauss action and log-prob of the draws eps, in fp64, each with a bound on what fp32
    evaluation may deviate: per layer (K + 2) u sum|W||h| (any summation order) + PROPAGATE sqrt(W^2 dh_in^2), GELU slope <= 1.13,
    then exp / tanh / log through their derivatives, plus the fp32 rounding of 1 + 1e-6 - t^2 near saturation"""
    h = obs.astype(np.float64)
    dh = np.zeros_like(h)
    for W, b, act in P["layers"]:
        aW = np.abs(W)
        z = h @ W.T + b
        # this layer's own rounding: worst case over every summation order. The incoming errors are independent roundings
        # of different units: they add in quadrature through W (a worst-case |W| sum would grow ~8x per 256-wide layer and
        # bury any stale weights); the worst-case local terms already sit ~sqrt(K) above the actual rounding
        dz = PROPAGATE * np.sqrt((dh * dh) @ (W * W).T) + (W.shape[1] + 2) * U * (np.abs(h) @ aW.T + np.abs(b))
        if act == "GELU":
            h = torch.nn.functional.gelu(torch.from_numpy(z)).numpy()
            dh = 1.13 * dz + 8 * U * (np.abs(z) + np.abs(h))
        else:
            h, dh = z, dz
    A = eps.shape[1]
    mean, dmean = h[:, :A], dh[:, :A]
    ls = np.clip(h[:, A:], *P["ls"])
    std = np.exp(ls)
    dstd = std * np.expm1(dh[:, A:]) + 4 * U * std
    e = eps.astype(np.float64)
    x = mean + e * std
    dx = dmean + np.abs(e) * dstd + 2 * U * (np.abs(mean) + 2 * np.abs(e * std))
    t = np.tanh(x)
    dt = (1 - t * t) * dx + 4 * U * np.abs(t)
    half, center = P["half"], P["center"]
    a = half * t + center
    da = np.abs(half) * dt + 4 * U * (np.abs(half * t) + np.abs(center))
    arg = 1 + LOG_EPS - t * t
    base = -0.5 * ((x - mean) / std) ** 2 - ls - np.log(np.sqrt(2 * np.pi))
    sq = -np.log(arg)
    lp = (base + sq).sum(-1) - np.log(half).sum()
    dlp = (dstd / std + 4 * U * (np.abs(ls) + 1) + np.abs(e) * 4 * U * (np.abs(x) + np.abs(mean)) / std + U * e * e
           + (3 * U + 2 * np.abs(t) * dt) / arg + 2 * U * np.abs(sq)).sum(-1)
    dlp = dlp + (2 * A + 2) * U * (np.abs(base).sum(-1) + np.abs(sq).sum(-1) + np.abs(np.log(half)).sum())
    lg = np.concatenate([mean, std], 1)
    dlg = np.concatenate([dmean, dstd], 1)
    return {"lg": lg, "dlg": SAFETY * dlg, "a": a, "da": SAFETY * da, "lp": lp, "dlp": SAFETY * dlp}


def _within(got, want, tol, tag):
    err = np.abs(np.asarray(got, np.float64) - want)
    bad = ~(err <= tol)
    assert not bad.any(), "%s: %d of %d values off the fp64 forward of the live weights (worst %.3g x the fp32 bound)" % (
        tag, int(bad.sum()), bad.size, float(np.max(err / tol)))


class Acting:
    """the acting routes of one handle, checked against the fp64 forward of the arena's weights after each event"""

    def __init__(self, alg, kw, seed=3, scale=1.0):
        self.alg, self.kw, self.e = alg, kw, alg.engine
        assert self.e.debug_get("act_host") == 1.0, "this handle does not act on the host"
        O, A = self.e.obs_dim, self.e.act_dim
        rng = np.random.default_rng(seed)
        self.obs = (scale * rng.standard_normal((N_ROWS, O))).astype(np.float32)
        self.eps = rng.standard_normal((N_ROWS, A)).astype(np.float32)
        self.P = _live_policy(alg, kw)
        self.ref = _fp64_policy(self.P, self.obs, self.eps)
        self.host_lg = None
        self.check("initial", moved=None)

    def settle(self):
        """one host acting call: whatever marked the snapshot stale (the host_act toggle, a torch write the module forward
        noticed) is consumed here, BEFORE the next event -- the next event's acting calls see only what that event did"""
        self.e.act_sample(self.obs[0], self.eps[0])
        return self.e.debug_get("act_copies")

    def guard(self, new, old, rows, tag):
        """the case can tell stale weights from live ones: some output of the previous weights is >= GUARD bounds away"""
        for k, dk in (("lg", "dlg"), ("a", "da")):
            r = float(np.max(np.abs(new[k][rows] - old[k][rows]) / new[dk][rows]))
            assert r >= GUARD, "%s: ill-posed -- the previous weights' %s are only %.3g bounds from the live ones" % (tag, k, r)

    def check(self, tag, moved=True, torch_write=False):
        """moved: True (the event changed the policy: separation guard), False (it must not have: bit-equal host logits),
        None (no previous state)"""
        e, obs, eps = self.e, self.obs, self.eps
        out = {}
        if torch_write:   # the documented noticing point for torch writes: the module forward reads the version counters
            out["module n=1"] = ("lg", slice(0, 1), self.alg.networks.policy(torch.from_numpy(obs[:1])).numpy())
        a, lp = e.act_sample(obs[0], eps[0])
        out["host act_sample"] = ("a", slice(0, 1), a.copy()[None], np.array([float(lp[0])]))
        out["host policy_forward"] = ("lg", slice(0, 1), e.policy_forward(obs[:1]).copy())
        if not torch_write:
            out["module n=1"] = ("lg", slice(0, 1), self.alg.networks.policy(torch.from_numpy(obs[:1])).numpy())
        for n in (1, 33, N_ROWS):
            a, lp = e.act_sample_batch(obs[:n], eps[:n])
            out["act_sample_batch n=%d" % n] = ("a", slice(0, n), a, lp)
        out["module n=40"] = ("lg", slice(0, 40), self.alg.networks.policy(torch.from_numpy(obs[:40])).numpy())
        host_lg = out["host policy_forward"][2]
        # the one-launch GPU forward, selected only now (the switch marks the snapshot stale)
        e.debug_set("host_act", 0)
        a, lp = e.act_sample(obs[0], eps[0])
        out["gpu act_sample"] = ("a", slice(0, 1), a.copy()[None], np.array([float(lp[0])]))
        out["gpu policy_forward"] = ("lg", slice(0, 1), e.policy_forward(obs[:1]).copy())
        e.debug_set("host_act", 1)
        P = _live_policy(self.alg, self.kw)
        ref = _fp64_policy(P, obs, eps)
        for route, (kind, rows, *got) in out.items():
            t = "%s / %s" % (tag, route)
            if kind == "lg":
                _within(got[0], ref["lg"][rows], ref["dlg"][rows], t + " logits")
            else:
                _within(got[0], ref["a"][rows], ref["da"][rows], t + " action")
                _within(got[1], ref["lp"][rows], ref["dlp"][rows], t + " log-prob")
        if moved:
            self.guard(ref, self.ref, slice(0, 1), tag)
        elif moved is False:
            assert np.array_equal(host_lg, self.host_lg), "%s: the policy moved on an update that leaves it alone" % tag
        self.P, self.ref, self.host_lg = P, ref, host_lg
        return self.settle()


def _policy_out_bias(alg):
    """the output layer's bias of the online policy: a contiguous window of engine.online"""
    p = list(alg.networks.policy.parameters())[-1]
    assert p.dim() == 1 and p.is_contiguous()
    return p


# ---- one handle, every single-process update entry point -------------------------------------------------------------
SHAPES = [
    pytest.param(376, 17, (256, 256, 256), 256, 0.4, id="humanoid"),     # the BASELINE policy
    pytest.param(5, 1, (33,), 16, 2.0, id="ragged"),
]


@pytest.mark.parametrize("O,A,hid,B,lim", SHAPES)
def test_single_process_update_paths(O, A, hid, B, lim, tmp_path):
    from dsac_v2_hip import HipBatchGroup

    kw = _kw(O, A, hid, B, lim, seed=5)
    alg = _make(kw, 4)
    e = alg.engine
    rows = _fill_ring(e, 1024)
    ac = Acting(alg, kw)
    # eager step on an iteration that leaves the policy alone (delay_update 2): no copy, bit-equal logits
    copies = ac.settle()
    e.gather(rows[0]); e.step(1)
    assert e.debug_get("act_copies") == copies
    copies = ac.check("eager step, off iteration", moved=False)
    # eager step that moves it: exactly one copy, enqueued by the update call itself
    e.gather(rows[1]); e.step(2)
    assert e.debug_get("act_copies") == copies + 1
    ac.check("eager step")
    e.gather(rows[2]); e.compute_grads(4); e.apply_update(4)
    ac.check("compute_grads + apply_update")
    # gradients from a second algorithm (the reference's remote seam)
    alg2 = _make(kw, 9)
    _, info = alg2.get_remote_update_info(_batch(np.random.default_rng(7), B, O, A, lim), 6)
    alg.remote_update(info)
    ac.check("remote_update")
    del info, alg2
    # local_update_group: aligned (one group replay), then with the skip-actor flag cut off the delay_update period
    alg.local_update_group(HipBatchGroup(e, rows[:4]), 8)
    ac.check("local_update_group aligned")
    alg.flags = SKIP_ACTOR
    alg.local_update_group(HipBatchGroup(e, rows[:5]), 13)      # head: it 13 (eager, off) -- body: 14..17 as one replay
    ac.check("local_update_group misaligned, body last")
    alg.local_update_group(HipBatchGroup(e, rows[:4]), 19)      # head: 19 -- body: 20, 21 -- tail: 22 (eager, moves)
    ac.check("local_update_group misaligned, tail last")
    alg.flags = 0
    e.run_group(24, rows[:4])
    ac.check("run_group")
    # graph_build alone (after an acting call) neither copies nor changes what acting returns; graph_run moves the policy
    for flags, it in ((0, 28), (SKIP_ACTOR, 36)):
        copies = ac.settle()
        e.graph_build(4, flags)
        assert e.debug_get("act_copies") == copies, "graph_build enqueued a snapshot copy (flags %d)" % flags
        ac.check("graph_build alone, flags %d" % flags, moved=False)
        e.graph_run(it, 8)
        ac.check("graph_run, flags %d" % flags)
    # load_state_dict, and the shipped checkpoint round trip (trainer: torch.save(networks.state_dict()) + the sidecar)
    sd = {k: v.clone() for k, v in alg.networks.state_dict().items()}
    for k in sd:
        if k.startswith("policy.policy.") and k.endswith("bias"):
            sd[k] += 0.05
    alg.networks.load_state_dict(sd)
    ac.check("load_state_dict")
    path = str(tmp_path / "apprfunc.pkl")
    torch.save(alg.networks.state_dict(), path)
    torch.save(alg.optimizer_state_dict(), path + ".opt")
    e.gather(rows[3]); e.step(44)
    ac.check("update after the checkpoint")
    alg.networks.load_state_dict(torch.load(path))
    alg.load_optimizer_state_dict(torch.load(path + ".opt"))
    ac.check("checkpoint restored")
    # torch writes: version counters the module forward (and the samplers) read
    p = _policy_out_bias(alg)
    with torch.no_grad():
        p.add_(0.05)
    torch.cuda.synchronize()
    ac.check("in-place p.add_ under no_grad", torch_write=True)
    off = p.storage_offset()
    with torch.no_grad():
        e.online[off:off + p.numel()] -= 0.07          # a slice write through the engine's own arena tensor
    torch.cuda.synchronize()
    ac.check("engine.online slice write", torch_write=True)
    # p.data.copy_ bypasses every counter: INTEGRATION.md's contract is an explicit policy_dirty(). The routes that read the
    # device arena see the write at once; the host snapshot follows the policy_dirty() call.
    p.data.copy_(p.data + 0.06)
    torch.cuda.synchronize()
    ref = _fp64_policy(_live_policy(alg, kw), ac.obs, ac.eps)
    a, lp = e.act_sample_batch(ac.obs[:33], ac.eps[:33])
    _within(a, ref["a"][:33], ref["da"][:33], "p.data.copy_ / act_sample_batch action")
    _within(lp, ref["lp"][:33], ref["dlp"][:33], "p.data.copy_ / act_sample_batch log-prob")
    lg = alg.networks.policy(torch.from_numpy(ac.obs[:40])).numpy()
    _within(lg, ref["lg"][:40], ref["dlg"][:40], "p.data.copy_ / module n=40 logits")
    e.policy_dirty()
    ac.check("p.data.copy_ + policy_dirty()")


def test_dsac_v1_eager_and_remote_update():
    O, A, hid, B, lim = 24, 6, (64, 64), 64, 0.4
    kw = _kw(O, A, hid, B, lim, algorithm="DSAC_V1_HIP", TD_bound=10.0, seed=5)
    alg = _make(kw, 5)
    rng = np.random.default_rng(11)
    ac = Acting(alg, kw)
    alg.local_update(_batch(rng, B, O, A, lim), 0)
    ac.check("DSAC_V1 local_update")
    alg2 = _make(kw, 6)
    _, info = alg2.get_remote_update_info(_batch(rng, B, O, A, lim), 2)
    alg.remote_update(info)
    ac.check("DSAC_V1 remote_update")


# ---- data parallel (world 1 over gloo; force_collective issues the all-reduce anyway) ----------------------------------
@pytest.fixture(scope="module")
def gloo_world1():
    import torch.distributed as dist

    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29547")
        dist.init_process_group("gloo", rank=0, world_size=1)
        created = True
    yield
    if created:
        dist.destroy_process_group()


DP = (16, 4, (64, 64), 64, 0.3)      # _ToyEnv's shape and action limit (the vectorised sampler case)


def _dp_handle(seed=4):
    O, A, hid, B, lim = DP
    kw = _kw(O, A, hid, B, lim, seed=5)
    alg = _make(kw, seed)
    _fill_ring(alg.engine, 1024)
    return alg, kw


def _updater(e, **kw):
    from dsact.dp import DataParallelUpdater

    dp = DataParallelUpdater(e, broadcast_tensors=(e.online, e.target, e.adam_m, e.adam_v), **kw)
    dp.force_collective = True
    return dp


def test_dp_broadcast_marks_the_snapshot_stale(gloo_world1):
    """the broadcast in DataParallelUpdater.__init__ writes the arenas past every version counter (with one rank it rewrites
    them in place; a write through p.data stands in for rank 0's values arriving)"""
    alg, kw = _dp_handle()
    ac = Acting(alg, kw)
    p = _policy_out_bias(alg)
    p.data.copy_(p.data + 0.06)
    torch.cuda.synchronize()
    _updater(alg.engine)
    ac.check("DataParallelUpdater broadcast")


@pytest.mark.parametrize("mode", ["eager", "overlapped", "strict"])
def test_dp_eager_apply(mode, gloo_world1):
    """dsact_dp_enqueue_apply refreshes the snapshot behind every apply. The device iteration decides whether the policy
    moved, so the copy is unconditional: on an iteration that leaves the policy alone it is redundant, which is accepted."""
    from training.hip_vec_sampler import HipVecOffSampler
    from test_hip_groups import _ToyEnv

    alg, kw = _dp_handle()
    e = alg.engine
    dp = _updater(e, overlap=mode == "overlapped", strict=mode == "strict")
    assert dp.overlap == (mode == "overlapped") and dp.strict == (mode == "strict")
    ac = Acting(alg, kw)
    e.dp_begin(0)
    dp.step()                                          # iteration 0: moves the policy
    ac.check("dp %s step" % mode)
    copies = ac.settle()
    dp.step()                                          # iteration 1: leaves it alone (one redundant copy)
    assert e.debug_get("act_copies") <= copies + 1
    ac.check("dp %s step, off iteration" % mode, moved=False)
    if mode != "eager":
        return
    # HipVecOffSampler after a data-parallel step, on both routes, row by row
    dp.step()                                          # iteration 2
    O, A = DP[0], DP[1]
    P = _live_policy(alg, kw)
    rows = np.random.default_rng(21).standard_normal((8, O)).astype(np.float32)
    for route in ("host", "gpu"):
        smp = HipVecOffSampler(envs=[_ToyEnv() for _ in range(8)], networks=alg.networks, sample_batch_size=8,
                               action_type="continu", hip_vec_act=route)
        assert smp.route() == route
        smp.obs[...] = rows
        torch.manual_seed(30)
        batch, _ = smp.sample()
        torch.manual_seed(30)
        eps = torch.randn(8, A).numpy()
        np.testing.assert_array_equal(batch.packed[0], rows)
        ref = _fp64_policy(P, rows, eps)
        prev = _fp64_policy(ac.P, rows, eps)
        tag = "HipVecOffSampler %s after a dp step" % route
        _within(batch.packed[1], ref["a"], ref["da"], tag + " action")
        _within(batch.packed[5], ref["lp"], ref["dlp"], tag + " log-prob")
        ac.guard(ref, prev, slice(0, 8), tag)


@pytest.mark.parametrize("flavour,strict,steps", [("pipelined", False, 2), ("merged", False, 1), ("non-merged", True, 2)])
def test_dp_native_graph(flavour, strict, steps, gloo_world1):
    """the native RCCL graph in its three captures: pipelined (the default), merged gather (one update per graph), and
    non-merged (strict std sums: capture_updates calls enqueue_graph_step_dp once per update). Building after an acting call
    neither copies nor changes what acting returns; graph_run refreshes the snapshot."""
    alg, kw = _dp_handle()
    e = alg.engine
    dp = _updater(e, native=True, strict=strict)
    ac = Acting(alg, kw)
    copies = ac.settle()
    assert dp.build_graph(steps, fallback=False)
    got = (e.debug_get("pipe_graph"), e.debug_get("merged_graph"))
    assert got == {"pipelined": (1.0, 1.0), "merged": (0.0, 1.0), "non-merged": (0.0, 0.0)}[flavour], got
    assert e.debug_get("act_copies") == copies, "the data-parallel graph build enqueued a snapshot copy"
    ac.check("dp graph_build alone (%s)" % flavour, moved=False)
    dp.run_graph(0, 4)
    ac.check("dp graph_run (%s)" % flavour)
    e.comm_destroy()


def test_load_state_dict_then_dp_graph_build(gloo_world1):
    """load_state_dict bumps the epoch without copying; a data-parallel graph build right after must not mark the old
    snapshot current"""
    alg, kw = _dp_handle()
    e = alg.engine
    dp = _updater(e, native=True)
    ac = Acting(alg, kw)
    sd = {k: v.clone() for k, v in alg.networks.state_dict().items()}
    for k in sd:
        if k.startswith("policy.policy.") and k.endswith("bias"):
            sd[k] -= 0.05
    alg.networks.load_state_dict(sd)
    assert dp.build_graph(2, fallback=False)
    ac.check("load_state_dict, then the dp graph build")
    e.comm_destroy()
