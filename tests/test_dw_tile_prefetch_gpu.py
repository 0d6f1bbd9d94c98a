"""The weight-gradient tiles (dw2_tile, csrc/dsact_chain.h) fetch the Adam / Polyak operands of their bias rows and of their
ragged quads (the last, partly valid group of four columns of a row whose width is no multiple of 4) in front of the wait for
their chain instead of after the contraction. Same addresses, same arithmetic, same stores: 8 updates (both parities of
delay_update = 2: Polyak on and off, policy tiles that apply and the deferred ones that apply nothing) must leave the online
and target arenas, both Adam moments and the 14 statistics
  * bitwise equal between the pipelined graph and eager updates (the project's launch-form method), and
  * equal to what the PARENT commit computed: SHA-256 digests in tests/golden/dw_tile_prefetch_parent.json, which names it.

Shapes: the smallest at which each changed path can go wrong --
  obs 11, act 3, 2x64, batch 16    critic first layer N = 14: a ragged quad of 2 valid columns, N < 32; output layers M = 2 / 6
  obs 17, act 6, 2x64, batch 32    N = 23: 3 valid columns
  obs 16, act 17, 2x128, batch 64  N = 33: 1 valid column in a second column block; M = 34 policy output rows (two bias row
                                   tiles). The graph's 8-row policy units add logp in another order than eager updates here
                                   (tests/test_bwd_dact_tail_gpu.py), so the graph is compared with its own launch sequence
                                   issued eagerly
  obs 376, act 17, 3x256, batch 256  the headline's own tile list: two updates, graph form, parent digest only
  DSAC_V1 (one critic) at obs 11, act 3, 2x64, batch 16

Recording (on the PARENT commit only, never from the code under test):
    python tests/test_dw_tile_prefetch_gpu.py OUT.json COMMIT"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dw_tile_prefetch_parent.json")
ARENAS = ("online", "target", "adam_m", "adam_v")
FIRST, N = 1, 512   # iterations 1 .. TOTAL, delay_update 2: even iterations move the policy

CASES = [
    # v1, O, A, hidden, B, updates, reference form of the graph
    (False, 11, 3, (64, 64), 16, 8, "eager"),
    (False, 17, 6, (64, 64), 32, 8, "eager"),
    (False, 16, 17, (128, 128), 64, 8, "sequence"),
    (False, 376, 17, (256, 256, 256), 256, 2, None),
    (True, 11, 3, (64, 64), 16, 8, "eager"),
]


def _case_id(v1, O, A, hid, B, total, ref):
    return "%s-O%d-A%d-h%s-B%d-u%d" % ("v1" if v1 else "v2", O, A, "x".join(str(h) for h in hid), B, total)


def _engine(v1, O, A, hid, B, total):
    if v1:
        from test_hip_v1_parity import make_pair as make_v1

        alg, _ = make_v1(O, A, hid, B, seed=6, delay_update=2)
    else:
        from test_hip_parity import make_pair

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
    e.upload_index_table(np.random.randint(0, N, size=(total + 3, B)))
    return alg


def _snapshot(alg):
    """(arenas, statistics, digests)"""
    e = alg.engine
    e.sync()
    st = {k: v for k, v in e.read_stats().items() if not k.startswith("_device")}
    assert len(st) >= 14, sorted(st)
    ar, dig = {}, {}
    for n in ARENAS:
        t = getattr(e, n).detach().cpu().contiguous()
        assert bool(torch.isfinite(t).all()), n
        ar[n] = t
        dig[n] = hashlib.sha256(t.numpy().tobytes()).hexdigest()
    keys = sorted(st)
    dig["stats"] = hashlib.sha256((",".join(keys) + "|").encode() + np.array([st[k] for k in keys], dtype=np.float32).tobytes()).hexdigest()
    return ar, st, dig


def run_case(v1, O, A, hid, B, total, ref):
    """{"graph" | ref: snapshot}, and the launch names of the pipelined sequence (None where it is not issued)"""
    snaps, names = {}, None
    for mode in ("graph", ref):
        if mode is None:
            continue
        alg = _engine(v1, O, A, hid, B, total)
        e = alg.engine
        if mode == "eager":
            assert e.time_steps(FIRST, total, use_graph=False) > 0
        elif mode == "sequence":   # the pipelined graph's launches issued one by one
            names = [n for n, _, _ in e.profile_steps(FIRST, total)]
        else:
            e.graph_build(total)
            assert e.debug_get("pipe_graph") == 1.0
            e.graph_run(FIRST, total)
        snaps[mode] = _snapshot(alg)
        assert e.debug_get("handoff_failures") == 0.0
    return snaps, names


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["parent_commit"]
    return g["cases"]


@pytest.mark.parametrize("v1,O,A,hid,B,total,ref", CASES, ids=[_case_id(*c) for c in CASES])
def test_prefetched_tile_operands_leave_the_update_bit_identical(v1, O, A, hid, B, total, ref, golden, monkeypatch):
    for k in ("DSACT_NO_BQT_MERGE", "DSACT_NO_BQP_MERGE"):
        monkeypatch.delenv(k, raising=False)
    want = golden[_case_id(v1, O, A, hid, B, total, ref)]
    snaps, names = run_case(v1, O, A, hid, B, total, ref)
    bad = []   # every mismatch, so that a failure says which form and which result differ
    if names is not None:
        print("launches:", sorted(set(names)))
        assert "chain_bwd_qt" in names and "chain_bwd_qpt" in names, names
    if ref is not None:
        ar0, st0, _ = snaps[ref]
        ar, st, _ = snaps["graph"]
        for n in ARENAS:
            if not torch.equal(ar0[n], ar[n]):
                bad.append(("graph != " + ref, n, float((ar0[n] - ar[n]).abs().max())))
        for k in st0:
            if not (st0[k] == st[k] or (np.isnan(st0[k]) and np.isnan(st[k]))):
                bad.append(("graph != " + ref, k, st0[k], st[k]))
    for mode in snaps:
        dig = snaps[mode][2]
        bad += [(mode + " != parent", k, dig[k], want[mode][k]) for k in want[mode] if dig[k] != want[mode][k]]
    assert not bad, "\n".join(str(b) for b in bad)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "tests"), os.path.join(root, "dsac-v2_amd"), root):
        if p not in sys.path:
            sys.path.insert(0, p)
    out_path, commit = sys.argv[1], sys.argv[2]
    cases = {}
    for c in CASES:
        snaps, names = run_case(*c)
        if c[-1] is not None:
            assert snaps["graph"][2] == snaps[c[-1]][2], (c, "the graph and its reference form differ on the recording commit")
        cases[_case_id(*c)] = {mode: snaps[mode][2] for mode in snaps}
        print(_case_id(*c), "recorded", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"parent_commit": commit, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path)
