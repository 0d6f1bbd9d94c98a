"""The merged backward launches (k_chain_bwd_qt / k_chain_bwd_qpt) fetch the dL/d action fragments of q(obs, new_act)'s first
layer in the drained tail of the last hidden product's weight stream (gemm44_seg<RG, TAIL>) instead of after the last epilogue.
Same addresses, same MFMA order: the pipelined graph must stay bit-identical to eager updates and to the launch forms that
do not take the tail (DSACT_NO_BQT_MERGE / DSACT_NO_BQP_MERGE: k_chain_bwd_q keeps its load beside the stream).

Shapes: the smallest at which the tail can go wrong -- one output tile of the narrow product (A = 3), exactly one (A = 16),
two (A = 17: all 8 slots), 1 / 2 / 4 waves per workgroup (widths 64 / 128 / 256: the fragment address depends on the wave), one
hidden layer (no stream: the fallback load), two and three (a product with a stream tail, with and without a successor
product before it), batch 16 and 64, odd and aligned observation widths, and DSAC_V1 (one critic)."""
import numpy as np
import pytest
import torch

from test_hip_parity import make_pair

pytestmark = pytest.mark.gpu

BUFFERS = ("d_new_act", "dZ.q1p.0", "dZ.pi.0")
ARENAS = ("online", "target", "adam_m", "adam_v")
FIRST, TOTAL, PER_GRAPH, N = 1, 8, 4, 512   # iterations 1 .. 8: the last update moves the policy (the whole backward is one launch)


def _engine(v1, O, A, hid, B):
    if v1:
        from test_hip_v1_parity import make_pair as make_v1

        alg, _ = make_v1(O, A, hid, B, seed=6, delay_update=2)
    else:
        alg, _ = make_pair(O, A, hid, B, seed=6, delay_update=2)
    e = alg.engine
    assert e.chain_active
    e.set_device_rng(321)
    e.buffer_create(N)
    g = torch.Generator(device="cuda").manual_seed(2)
    e.buffer_fill_device(0, torch.randn(N, O, device="cuda", generator=g), torch.rand(N, A, device="cuda", generator=g) - .5,
                         torch.randn(N, device="cuda", generator=g), torch.randn(N, O, device="cuda", generator=g),
                         (torch.rand(N, device="cuda", generator=g) < .05).float())
    np.random.seed(3)
    e.upload_index_table(np.random.randint(0, N, size=(5, B)))
    return alg


def _snapshot(alg):
    e = alg.engine
    e.sync()
    st = {k: v for k, v in e.read_stats().items() if not k.startswith("_device")}
    return ({n: getattr(e, n).clone() for n in ARENAS}, {n: e.debug_read(n) for n in BUFFERS}, st, e.get_state())


@pytest.mark.parametrize("v1,O,A,hid,B", [
    (False, 11, 3, (64, 64), 16),            # one output tile, one wave, smallest batch, odd observation width
    (False, 16, 16, (128, 128, 128), 64),    # exactly one tile, two waves, three layers
    (False, 11, 17, (256, 256), 64),         # two tiles (8 slots), four waves, the tail follows the stream's prologue directly
    (False, 16, 17, (256, 256, 256), 16),    # two tiles, four waves, three layers, batch 16
    (False, 16, 17, (128, 128), 64),         # two tiles, two waves
    (False, 11, 3, (64,), 64),               # one hidden layer: no stream, the fallback load
    (False, 16, 17, (256,), 16),             # ... with two tiles and four waves
    (True, 11, 3, (64, 64), 64),             # DSAC_V1: one critic
])
def test_tail_fetched_fragments_leave_every_launch_form_bit_identical(v1, O, A, hid, B, monkeypatch):
    snaps, names = {}, None
    for mode in ("eager", "graph", "sequence", "no_bqt", "no_bqp"):
        for k in ("DSACT_NO_BQT_MERGE", "DSACT_NO_BQP_MERGE"):
            monkeypatch.delenv(k, raising=False)
        if mode == "no_bqt":
            monkeypatch.setenv("DSACT_NO_BQT_MERGE", "1")
        if mode == "no_bqp":
            monkeypatch.setenv("DSACT_NO_BQP_MERGE", "1")
        alg = _engine(v1, O, A, hid, B)
        e = alg.engine
        if mode == "eager":
            assert e.time_steps(FIRST, TOTAL, use_graph=False) > 0
        elif mode == "sequence":   # the pipelined graph's launches issued one by one: their names
            names = [n for n, _, _ in e.profile_steps(FIRST, TOTAL)]
        else:
            e.graph_build(PER_GRAPH)
            assert e.debug_get("pipe_graph") == 1.0
            e.graph_run(FIRST, TOTAL)
        snaps[mode] = _snapshot(alg)
        assert e.debug_get("handoff_failures") == 0.0
    # the merged launches are what the default form runs (their tail is the code under test)
    assert "chain_bwd_qt" in names, names
    if not v1:
        assert "chain_bwd_qpt" in names, names
    # Eager updates are bit-comparable with the pipelined graph only while one lane holds one action dimension in the policy
    # head's row phase: the graph runs the NEXT minibatch's policy units as 8-row workgroups (64 * NW / 8 lanes per row), and
    # with more action dimensions than that a lane adds two log-prob terms before the row's lanes are summed -- another
    # (equally valid) summation order than the 4-row workgroups of an eager update, in the forward, whatever the backward does.
    # Such a shape (two waves x 17 actions: 17 > 16) still compares every launch form of the graph with every other one --
    # the merged launches (tail) against the unmerged ones (k_chain_bwd_q: load beside the stream).
    eager_comparable = A <= 64 * (hid[0] // 64) // 8
    ref = "eager" if eager_comparable else "graph"
    ar0, buf0, st0, state0 = snaps[ref]
    assert len(st0) >= 14, sorted(st0)
    for n in ARENAS:
        assert bool(torch.isfinite(ar0[n]).all()), n
    bad = []   # every mismatch, so that a failure says which launch forms and which results differ
    for mode in ("graph", "sequence", "no_bqt", "no_bqp"):
        if mode == ref:
            continue
        ar, buf, st, state = snaps[mode]
        for n in ARENAS:
            if not torch.equal(ar0[n], ar[n]):
                bad.append((mode, n, float((ar0[n] - ar[n]).abs().max())))
        for n in BUFFERS:
            if not np.array_equal(buf0[n], buf[n]):
                bad.append((mode, n, float(np.abs(buf0[n] - buf[n]).max())))
        for k in st0:
            if not (st0[k] == st[k] or (np.isnan(st0[k]) and np.isnan(st[k]))):
                bad.append((mode, k, st0[k], st[k]))
        if state0 != state:
            bad.append((mode, "state"))
    print("launches:", sorted(set(names)))
    assert not bad, "\n".join(str(b) for b in bad)
