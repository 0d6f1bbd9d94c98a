"""The per-sample glue of the loss, in every hand-written copy, driven into its clamps, ties and thresholds.

k_loss (tile stages), the row phase of the backward chains (all launch forms), the throughput regime's row phase and the
DSAC_V1 variants each restate min / where, the +-3 clamp on z, softplus and its threshold, the variance-ratio clamp, the Huber
branches, the actor's tie weight and the log-std gate. The benign parity inputs reach none of those branches
(tests/stress_cases.py); these cases do, through the unchanged run_case of tests/test_hip_parity.py / test_hip_v1_parity.py and
its unchanged gates. tests/test_loss_regimes_host.py holds the contract of every case used here: rows per regime at each of the
3 updates, and the oracle's own fp32 rounding inside a quarter of every gate.
"""
import numpy as np
import pytest
import torch

import test_hip_parity as v2
import test_hip_v1_parity as v1
from stress_cases import ACT_LIMIT, RF, STEPS, V1_CASES, V2_CASES, case_kwargs, make_oracle, prepare_hook
from test_hip_parity import PIPE_BUFFERS

pytestmark = pytest.mark.gpu

TANH, GAUSS = "TanhGaussDistribution", "GaussDistribution"
TILE, CHAIN, HEADLINE = (11, 6, (96, 40), 64), (24, 6, (128, 128), 64), (376, 17, (256, 256, 256), 256)
FAT_FWD, FAT = (11, 6, (128, 128), 512), (11, 6, (128, 128), 4096)
# path -> (shape, chain_active, debug_get("fat"): 1 = throughput-regime forward, +2 = its backward (the row phase of dsact_fat.h), env)
PATHS = {
    "tile": (TILE, False, 0.0, {}),
    "chain": (CHAIN, True, 0.0, {}),
    "headline": (HEADLINE, True, 0.0, {}),
    "fat_fwd": (FAT_FWD, True, 1.0, {"DSACT_FAT_MIN": "512"}),
    "fat": (FAT, True, 3.0, {}),
}


def assert_path_and_ties(mod, path, init, inputs, kw, ties):
    """the kernel family the shape is meant to select IS selected; twin case: the twin chains give equal bits on the device at
    every update (they run the same code on the same bits), so that the tie is a tie for the kernels too"""
    (O, A, hid, B), chain, fat, _ = PATHS[path]
    alg, _ = mod.make_pair(O, A, hid, B, act_limit=ACT_LIMIT, init=init, **kw)
    e = alg.engine
    assert e.chain_active == chain, path
    assert e.debug_get("fat") == fat, (path, e.debug_get("fat"))
    if ties:
        for it, (data, noise) in enumerate(inputs):
            e.load_batch(*(data[k].numpy() for k in ("obs", "act", "rew", "obs2", "done")))
            e.set_noise(noise["eps_new"].numpy(), noise["eps_2"].numpy(), noise["z5"].numpy(), noise["z6"].numpy())
            e.compute_grads(it)
            e.sync()
            for a, b in (("qout_p0", "qout_p1"), ("qout_t0", "qout_t1")):
                x, y = e.debug_read(a), e.debug_read(b)
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (path, it, a, b, float(np.abs(x - y).max()))
            e.apply_update(it)
            e.sync()
    e.close()


def run_stressed(path, case, dist=TANH, monkeypatch=None):
    shape, _, _, env = PATHS[path]
    O, A, hid, B = shape
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    orc, inputs = make_oracle(case, shape, dist)
    init = orc.state_dict()
    kw = case_kwargs(case)
    if dist != TANH:
        kw["policy_act_distribution"] = dist
    assert_path_and_ties(v2, path, init, inputs, kw, ties=case == "twin")
    v2.run_case("regimes %s %s O=%d A=%d %s B=%d%s" % (path, case, O, A, hid, B, " Gauss" if dist != TANH else ""), O, A, hid, B,
                steps=STEPS, act_limit=ACT_LIMIT, init=init, prepare=prepare_hook(inputs),
                resync_last=case in ("spread", "threshold", "overflow"), **kw)
    for k in env:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("case", V2_CASES)
@pytest.mark.parametrize("path", ["tile", "chain", "fat_fwd", "fat"])
def test_stressed_parity(path, case, monkeypatch):
    """tile stages (k_heads, k_loss, k_heads_bwd), row-slice chains, the throughput regime's forward over the chains' backward
    (batch 512 with DSACT_FAT_MIN=512) and the throughput regime's own backward row phase (batch >= 4096)"""
    run_stressed(path, case, monkeypatch=monkeypatch)


@pytest.mark.parametrize("case", ["spread", "logstd"])
def test_stressed_parity_headline_shape(case):
    """the shipped <4, ...> chain instances at the BASELINE shape"""
    run_stressed("headline", case)


@pytest.mark.parametrize("path", ["tile", "chain"])
def test_stressed_parity_gauss_distribution(path):
    """GaussDistribution: the s == 0 branch of tanh_gauss_bwd has its own log-std gate"""
    run_stressed(path, "logstd", dist=GAUSS)


@pytest.mark.parametrize("case", V1_CASES)
@pytest.mark.parametrize("path", ["tile", "chain"])
def test_stressed_parity_v1(path, case):
    """DSAC_V1: k_loss_v1 and the a.v1 branch of the chains' row phase -- the log-std gate, TD_bound's clamp populated on both
    sides and inside, and the same rewards through the bound=False branch"""
    shape = PATHS[path][0]
    O, A, hid, B = shape
    orc, inputs = make_oracle(case, shape, v1=True)
    kw = case_kwargs(case, v1=True)
    alg, _ = v1.make_pair(O, A, hid, B, act_limit=ACT_LIMIT, init=orc.state_dict(), **kw)
    assert alg.engine.chain_active == PATHS[path][1]
    alg.engine.close()
    v1.run_case("regimes v1 %s %s O=%d A=%d %s B=%d" % (path, case, O, A, hid, B), O, A, hid, B, steps=STEPS, act_limit=ACT_LIMIT,
                init=orc.state_dict(), prepare=prepare_hook(inputs), **kw)


# ---- launch forms in the stressed regimes -----------------------------------------------------------------------------------
def _stressed_engine(case, seed=4):
    O, A, hid, B = CHAIN
    alg, _ = v2.make_pair(O, A, hid, B, act_limit=ACT_LIMIT, seed=seed, init=make_oracle(case, CHAIN)[0].state_dict(), delay_update=2,
                          **case_kwargs(case))
    e = alg.engine
    assert e.chain_active
    N = 2048
    e.set_device_rng(777)
    e.buffer_create(N)
    g = torch.Generator(device="cuda").manual_seed(1)
    e.buffer_fill_device(0, torch.randn(N, O, device="cuda", generator=g), torch.rand(N, A, device="cuda", generator=g) - .5,
                         RF * torch.randn(N, device="cuda", generator=g), torch.randn(N, O, device="cuda", generator=g),
                         (torch.rand(N, device="cuda", generator=g) < .05).float())
    np.random.seed(1)
    e.upload_index_table(np.random.randint(0, N, size=(7, B)))
    return alg


def _assert_same_bits(algs, stats, bufs):
    for other in range(1, len(algs)):
        for name in ("online", "target", "adam_m", "adam_v"):
            assert torch.equal(getattr(algs[0].engine, name), getattr(algs[other].engine, name)), (other, name)
        assert algs[0].engine.get_state() == algs[other].engine.get_state()
        assert torch.isfinite(algs[other].engine.online).all()
        for k in stats[0]:
            assert stats[0][k] == stats[other][k] or (np.isnan(stats[0][k]) and np.isnan(stats[other][k])), (other, k, stats[0][k], stats[other][k])
        for n in PIPE_BUFFERS:
            assert np.array_equal(bufs[0][n], bufs[other][n]), (other, n)
        b0, b1 = algs[0].engine.read_batch(with_logp=False), algs[other].engine.read_batch(with_logp=False)
        for k in ("obs", "act", "rew", "obs2", "done"):
            assert np.array_equal(b0[k], b1[k]), (other, k)


@pytest.mark.parametrize("case", ["spread+logstd", "twin"])
def test_graph_replay_equals_eager_steps_stressed(case):
    """test_graph_replay_equals_eager_steps with stressed nets (spread and logstd combined; twin alone) and ring rewards x RF:
    graph replays == eager updates, bit for bit, from iteration 0 with an odd number of updates per graph"""
    per_graph, total = 3, 6
    algs, stats, bufs = [], [], []
    for mode in ("eager", "graph"):
        alg = _stressed_engine(case)
        e = alg.engine
        if mode == "graph":
            e.graph_build(per_graph)
            e.graph_run(0, total)
        else:
            assert e.time_steps(0, total, use_graph=False) > 0
        e.sync()
        algs.append(alg)
        stats.append({k: v for k, v in e.read_stats().items() if not k.startswith("_device")})
        bufs.append({n: e.debug_read(n) for n in PIPE_BUFFERS})
    assert algs[1].engine.get_state()["adam_steps"] == [total, (total + 1) // 2, (total + 1) // 2]
    _assert_same_bits(algs, stats, bufs)


@pytest.mark.parametrize("case", ["spread+logstd", "twin"])
def test_pipelined_graph_equals_eager_steps_stressed(case):
    """test_pipelined_graph_equals_eager_steps with the same stressed nets and rewards: the merged launches (k_chain_bwd_qt,
    k_chain_bwd_qpt, k_chain_fwdpb) are separate instantiations of the row phase -- eager == pipelined graph == the same launch
    sequence issued eagerly, bit for bit, from an odd first iteration"""
    per_graph, first, total = 4, 1, 8
    algs, stats, bufs = [], [], []
    for mode in ("eager", "graph", "sequence"):
        alg = _stressed_engine(case)
        e = alg.engine
        if mode == "graph":
            e.graph_build(per_graph)
            assert e.debug_get("pipe_graph") == 1.0
            e.graph_run(first, total)
        elif mode == "sequence":
            names = [n for n, _, _ in e.profile_steps(first, total)]
            assert "chain_fwd+next" in names and "chain_bwd_qt" in names and "chain_bwd_qpt" in names, names
        else:
            assert e.time_steps(first, total, use_graph=False) > 0
        e.sync()
        algs.append(alg)
        stats.append({k: v for k, v in e.read_stats().items() if not k.startswith("_device")})
        bufs.append({n: e.debug_read(n) for n in PIPE_BUFFERS})
    _assert_same_bits(algs, stats, bufs)
