"""The chain kernels' inner product (gemm44_seg, csrc/dsact_chain.h) may fetch its LDS operand several steps ahead, fill the
accumulator hazard slot with a load and address the weight stream from scalar bases -- none of which changes which MFMA adds
what to which accumulator. So 8 updates must leave the parameters, the Adam moments and the statistics BIT-identical to what
the parent commit computed: SHA-256 digests recorded on the parent (tests/golden/gemm44_step_parent.json, which names it), for
eager updates and for the pipelined graph.

Shapes: the smallest at which a deeper operand ring or the new addressing can go wrong -- widths 64 (a product is exactly one
trip: the last trip is the first, the ring crosses the segment end at once) with one (no successor stream), two and three
hidden layers; 128 and 256 (two / four waves, two / four trips); observation widths 11 (odd, padded to one trip), 64 (exactly
one trip) and 80 (a second trip that is mostly padding); action widths 3 and 17; batch 16 and 64; batch 256 at (64, 64), where
eager updates take the 8-row form (n_units * B / 4 > 256); one DSAC_V1 case. In every case the graph runs the next
minibatch's policy units as 8-row workgroups and the merged backward launches run gemm44_seg<RG, TAIL>.

Recording (on the PARENT commit only, never from the code under test):
    python tests/test_gemm44_step_gpu.py OUT.json COMMIT"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm44_step_parent.json")
ARENAS = ("online", "target", "adam_m", "adam_v")
FIRST, TOTAL, PER_GRAPH, N = 1, 8, 4, 512   # iterations 1 .. 8, delay_update 2: the last update moves the policy

CASES = [
    # v1, O, A, hidden, B
    (False, 11, 3, (64,), 16),               # one layer: no successor stream; one trip
    (False, 64, 3, (64,), 64),               # ... with an observation of exactly one trip
    (False, 64, 17, (64, 64), 64),           # one trip per product, two action tiles (all 8 tail slots)
    (False, 80, 3, (64, 64, 64), 16),        # three layers of one trip; observation: second trip mostly padding
    (False, 11, 17, (128, 128), 64),         # two waves, two trips
    (False, 80, 17, (256, 256, 256), 16),    # four waves, four trips, three layers
    (False, 64, 3, (256, 256, 256), 64),     # ... at batch 64
    (False, 11, 3, (64, 64), 256),           # batch 256: the 8-row eager form
    (True, 11, 3, (64, 64), 64),             # DSAC_V1: one critic
]


def _case_id(v1, O, A, hid, B):
    return "%s-O%d-A%d-h%s-B%d" % ("v1" if v1 else "v2", O, A, "x".join(str(h) for h in hid), B)


def _engine(v1, O, A, hid, B):
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
    e.upload_index_table(np.random.randint(0, N, size=(5, B)))
    return alg


def _digests(alg):
    e = alg.engine
    e.sync()
    st = {k: v for k, v in e.read_stats().items() if not k.startswith("_device")}
    assert len(st) >= 14, sorted(st)
    out = {}
    for n in ARENAS:
        t = getattr(e, n)
        assert bool(torch.isfinite(t).all()), n
        out[n] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    keys = sorted(st)
    out["stats"] = hashlib.sha256((",".join(keys) + "|").encode() + np.array([st[k] for k in keys], dtype=np.float32).tobytes()).hexdigest()
    return out


def run_case(v1, O, A, hid, B):
    """{"eager" | "graph" | "sequence": digests}, and the launch names of the pipelined sequence"""
    got, names = {}, None
    for mode in ("eager", "graph", "sequence"):
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
        got[mode] = _digests(alg)
        assert e.debug_get("handoff_failures") == 0.0
    return got, names


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["parent_commit"]
    return g["cases"]


@pytest.mark.parametrize("v1,O,A,hid,B", CASES, ids=[_case_id(*c) for c in CASES])
def test_eight_updates_match_the_parent_commit_bit_for_bit(v1, O, A, hid, B, golden, monkeypatch):
    for k in ("DSACT_NO_BQT_MERGE", "DSACT_NO_BQP_MERGE"):
        monkeypatch.delenv(k, raising=False)
    want = golden[_case_id(v1, O, A, hid, B)]
    got, names = run_case(v1, O, A, hid, B)
    # the merged launches (gemm44_seg<RG, TAIL>) and the pipelined forward are what the default form runs
    assert "chain_bwd_qt" in names, names
    if not v1:
        assert "chain_bwd_qpt" in names, names
    print("launches:", sorted(set(names)))
    bad = [(mode, k, got[mode][k], want[ref][k]) for mode, ref in (("eager", "eager"), ("graph", "graph"), ("sequence", "graph"))
           for k in want[ref] if got[mode][k] != want[ref][k]]
    assert not bad, "\n".join(str(b) for b in bad)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "tests"), os.path.join(root, "dsac-v2_amd"), root):
        if p not in sys.path:
            sys.path.insert(0, p)
    out_path, commit = sys.argv[1], sys.argv[2]
    cases = {}
    for c in CASES:
        got, names = run_case(*c)
        assert got["sequence"] == got["graph"], (c, "the sequence and the graph differ on the recording commit")
        assert "chain_bwd_qt" in names, names
        cases[_case_id(*c)] = {"eager": got["eager"], "graph": got["graph"]}
        print(_case_id(*c), "recorded", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"parent_commit": commit, "updates": TOTAL, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path)
