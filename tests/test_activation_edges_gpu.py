"""Every forward path's activation epilogue, h = act(z) AND the stored derivative g = act'(z), across its breakpoints and tails.

The parity cases feed the epilogues |z| < 3 and compare the stored derivative with nothing. Here the nets are built so that every
hidden pre-activation is known exactly (tests/activation_sweep.py: one-hot first layers on observation rows that hold the sweep
table, diagonal +-2^k layers behind them, judged on the device's own stored h of the layer before), and H / G of every chain are
held to a float64 reference at |got - ref| <= 1e-6 + 2e-5 |ref|:

  the update's forward paths   tile stages, row-slice chains of width 64 / 128 / 256 (two launches and the merged launch), the
                               throughput-regime forward with two waves, 16-row and 32-row workgroups
  the acting forms             host route, one launch, the stand-alone tile-stage forward, act_sample_batch, act_mode_batch
  the output activations       policy_output_activation on the acting forms, value_output_activation on q(obs, act)

tests/test_activation_edges_host.py is the contract (table, reference, coverage of the deeper layers, mutation table)."""
import numpy as np
import pytest
import torch

import activation_sweep as sw
from test_hip_parity import _chains, _throughput, _tiles, make_pair

pytestmark = pytest.mark.gpu

DIFF, TARGET = ("pi", "q1c", "q2c", "q1p", "q2p"), ("pit", "q1t", "q2t")


def _fat3(e):
    assert e.chain_active and e.debug_get("fat") == 3.0


def reference_unique(act, z):
    """sw.reference on the distinct bit patterns of z (the rows of a large batch repeat the table)"""
    z = np.asarray(z, np.float32)
    u, inv = np.unique(z.view(np.uint32).reshape(-1), return_inverse=True)
    h, g = sw.reference(act, u.view(np.float32))
    return h[inv].reshape(z.shape), g[inv].reshape(z.shape)


def sweep_engine(O, A, hid, B, act, expect, **over):
    alg, _ = make_pair(O, A, hid, B, value_hidden_activation=act, policy_hidden_activation=act, **over)
    e = alg.engine
    expect(e)
    alg.networks.load_state_dict(sw.sweep_state(alg.networks.state_dict(), O))
    return alg


def load_sweep_batch(e, O, A, B):
    obs, obs2 = sw.sweep_obs(B, O), sw.sweep_obs(B, O, sw.OBS2_SHIFT)
    i = np.arange(B * A, dtype=np.float32).reshape(B, A)
    e.load_batch(obs, (0.3 * np.cos(i)).astype(np.float32), np.ones(B, np.float32), obs2, np.zeros(B, np.float32))
    r = np.arange(B, dtype=np.float32)
    e.set_noise(np.sin(i).astype(np.float32), np.cos(0.7 * i).astype(np.float32), np.sin(0.3 * r).astype(np.float32),
                np.cos(0.9 * r).astype(np.float32))
    return obs, obs2


def read_layer(e, name, B, w):
    """[B, w] of a hidden-layer buffer; the padded features behind w must be exact zeros"""
    got = e.debug_read(name, cap=B * 1024).reshape(B, -1)
    assert not got[:, w:].any(), "%s: the padded features are not zero" % name
    return got[:, :w]


def check_update_forward(e, path, act, O, A, hid, B):
    """one compute_grads(0); H and G of the differentiated chains, H of the target chains, every hidden layer. Returns
    {(kind, chain, layer): bits} for the launch-form comparisons and prints the worst error / gate of the case"""
    obs, obs2 = load_sweep_batch(e, O, A, B)
    e.compute_grads(0)
    e.sync()
    assert torch.isfinite(e.grads).all()
    table_bits = set(sw.table().view(np.uint32).tolist())
    worst, bits, cover = {"H": (0.0, None), "G": (0.0, None)}, {}, {}
    for ch in DIFF + TARGET:
        z = sw.z_layer0(obs2 if ch in TARGET else obs, hid[0])
        for l, w in enumerate(hid):
            if l:            # z_l = +-2^k h_{l-1}, exact on the device's own stored h_{l-1}
                z = sw.z_deeper(H, w)
                assert np.isfinite(z).all(), (path, act, ch, l)
            u, inv = np.unique(z.view(np.uint32).reshape(-1), return_inverse=True)     # (the rows of a large batch repeat the table)
            if l == 0:       # every table point reaches layer 0 of every chain
                assert table_bits <= set(u.tolist()), (path, act, ch)
            else:            # distinct pre-activations per interval of the activation's definition
                c = sw.assert_coverage(act, u.view(np.float32), "%s %s layer %d" % (path, ch, l))
                cover[l] = {k: min(v, cover.get(l, c)[k]) for k, v in c.items()}
            ref_h, ref_g = (r[inv].reshape(z.shape) for r in sw.reference(act, u.view(np.float32)))
            H = read_layer(e, "H.%s.%d" % (ch, l), B, w)
            kinds = [("H", H, ref_h)]
            if ch in DIFF:
                kinds.append(("G", read_layer(e, "G.%s.%d" % (ch, l), B, w), ref_g))
            for kind, got, ref in kinds:
                r, i = sw.worst(got, ref)
                if r > worst[kind][0]:
                    worst[kind] = (r, (ch, l, float(z.reshape(-1)[i])))
                bits[(kind, ch, l)] = got.view(np.uint32).copy()
    print("edges update %-9s %-8s B=%-5d H %.4f %s  G %.4f %s  least distinct points per interval, deeper layers %s" % (
        path, act, B, worst["H"][0], worst["H"][1], worst["G"][0], worst["G"][1], cover))
    for kind in "HG":
        assert worst[kind][0] <= 1.0, (path, act, kind, worst[kind])
    return bits


UPDATE_CASES = [(name, act) for name, spec in sw.UPDATE_SHAPES.items() for act in spec[4]]
EXPECT = {"tile": _tiles, "chain64": _chains, "chain128": _chains, "chain256": _chains, "fat_fwd": _throughput, "fat16": _throughput,
          "fat32": _fat3}


@pytest.mark.parametrize("path,act", UPDATE_CASES)
def test_update_forward_paths(path, act, monkeypatch):
    """tile stages (scalar act_fwd_grad / act4), row-slice chains (gelu4 / act4, dsact_chain.h), the throughput-regime forward
    (dsact_fat.h): two waves at batch 512 with DSACT_FAT_MIN=512, 16-row workgroups at batch 1024, 32-row ones at 4096"""
    O, A, hid, B, _ = sw.UPDATE_SHAPES[path]
    if path == "fat_fwd":
        monkeypatch.setenv("DSACT_FAT_MIN", "512")
    alg = sweep_engine(O, A, hid, B, act, EXPECT[path])
    monkeypatch.delenv("DSACT_FAT_MIN", raising=False)
    check_update_forward(alg.engine, path, act, O, A, hid, B)
    alg.engine.close()


@pytest.mark.parametrize("act", ["gelu", "selu"])
def test_merged_forward_launch_equals_two_launches_over_the_table(act):
    """k_chain_fwd2 (one launch, the policy in 4-row slices) and the two launches it replaces: both at the gate, and H / G bit
    for bit the same"""
    O, A, hid, B, _ = sw.UPDATE_SHAPES["chain64"]
    alg = sweep_engine(O, A, hid, B, act, _chains)
    e = alg.engine
    bits = []
    for merged in (0.0, 1.0):
        e.debug_set("fwd_merge", merged)
        assert e.debug_get("fwd_merge") == merged
        bits.append(check_update_forward(e, "merge=%d" % merged, act, O, A, hid, B))
    assert bits[0].keys() == bits[1].keys()
    for k in bits[0]:
        assert np.array_equal(bits[0][k], bits[1][k]), k
    e.close()


# ---- the acting forms -------------------------------------------------------------------------------------------------------
ACT_LIMIT = 2.0 ** 21          # GaussDistribution.mode() clamps the mean to the action limits: keep them outside the table
N_ROWS = 300


def acting_engine(hidden_act, out_act="linear"):
    O, A, hid = sw.ACTING_SHAPE
    alg, _ = make_pair(O, A, hid, 64, act_limit=ACT_LIMIT, policy_act_distribution="GaussDistribution",
                       value_hidden_activation=hidden_act, policy_hidden_activation=hidden_act, policy_output_activation=out_act)
    e = alg.engine
    assert e.debug_get("act_host") == 1.0 and e.debug_get("act_fast") == 1.0
    e.debug_set("mode_host_rows", 0)      # act_mode_batch: the batched launch at every row count
    return alg


def acting_means(e, obs, single_rows):
    """the mean columns of every acting form: {form: float32[rows, A]}; the batched forms over all of obs, the batch-1 forms
    over its first single_rows rows"""
    O, A, _ = sw.ACTING_SHAPE
    out = {}
    for name, host in (("host", 1), ("one_launch", 0)):
        e.debug_set("host_act", host)
        assert e.debug_get("act_host") == float(host)
        out[name] = np.concatenate([e.policy_forward(obs[i:i + 1])[:, :A] for i in range(single_rows)])
    e.debug_set("host_act", 1)
    out["forward"] = e.policy_forward(obs)[:, :A].copy()                      # chunks of 64 rows through the tile stages
    calls = e.debug_get("act_batch_calls"), e.debug_get("act_mode_calls")
    out["sample"] = e.act_sample_batch(obs, np.zeros((obs.shape[0], A), np.float32))[0]      # eps = 0: the action IS the mean
    out["mode"] = e.act_mode_batch(obs)
    assert e.debug_get("act_batch_calls") > calls[0] and e.debug_get("act_mode_calls") > calls[1]
    return out


def assert_batched_forms_agree(m, what):
    # (value equality: the sample is mean + 0 * sigma, which turns a mean of -0 into +0)
    assert np.array_equal(m["sample"], m["mode"]), what
    assert np.array_equal(m["forward"], m["sample"]), what
    n1 = m["one_launch"].shape[0]
    assert np.array_equal(m["one_launch"], m["sample"][:n1]), what


@pytest.mark.parametrize("act", sw.ACTS)
def test_acting_forms(act):
    """The output layer is one-hot: mean[r, a] IS the last hidden layer's stored feature col(a), and col(a) rotates until every
    feature has been read. Two families of nets, as on the host (test_activation_edges_host.py): the last hidden layer with zero
    weights and a slice of the table as its bias -- its pre-activation is exact, every table point is judged on every form --
    and the observation-driven chain with +-1 diagonals (layer 0 at the table, seen through layer 1)."""
    O, A, hid = sw.ACTING_SHAPE
    alg = acting_engine(act)
    e = alg.engine
    template = alg.networks.state_dict()
    obs = sw.sweep_obs(N_ROWS, O)
    single = -(-sw.table().size // O)
    ref_obs, z_last = sw.composed_reference(act, obs, hid)
    worst, judged = {}, set()
    for rot in range(-(-hid[-1] // A)):
        cols = sw.head_cols(A, hid[-1], rot)
        head = {"policy": sw.one_hot_head(A, hid[-1], rot)}
        for s, zb in enumerate(sw.bias_slices(hid[-1])):
            alg.networks.load_state_dict(sw.sweep_state(template, O, head=head, unit=True, last_bias={"policy": zb}))
            m = acting_means(e, obs, 2)
            assert_batched_forms_agree(m, (act, rot, s))
            want = sw.reference(act, zb[cols])[0]
            for form, got in m.items():
                assert np.array_equal(got, np.broadcast_to(got[:1], got.shape)), (form, act, rot, s)     # every row: the bias
                r, i = sw.worst(got[0], want)
                assert r <= 1.0, ("bias", form, act, rot, s, r, float(zb[cols][i]))
                worst[("bias", form)] = max(worst.get(("bias", form), 0.0), r)
            judged |= set(zb[cols].view(np.uint32).tolist())
        alg.networks.load_state_dict(sw.sweep_state(template, O, head=head, unit=True))
        m = acting_means(e, obs, single)
        assert_batched_forms_agree(m, (act, rot, "obs"))
        for form, got in m.items():
            want = ref_obs[:got.shape[0]][:, cols]
            r, i = sw.worst(got, want)
            assert r <= 1.0, ("obs", form, act, rot, r, float(z_last[:got.shape[0]][:, cols].reshape(-1)[i]))
            worst[("obs", form)] = max(worst.get(("obs", form), 0.0), r)
    assert judged == set(sw.table().view(np.uint32).tolist())
    print("edges acting %-8s %s" % (act, "  ".join("%s/%s %.4f" % (k[0], k[1], v) for k, v in sorted(worst.items()))))
    e.close()


# ---- output activations, forward values ---------------------------------------------------------------------------------------
def _relu_chain(obs, w):
    """stored features of a relu net with +1 diagonals: relu(obs[:, j mod O]), exact"""
    return np.maximum(sw.z_layer0(obs, w), np.float32(0.0))


@pytest.mark.parametrize("out_act", sw.ACTS)
def test_policy_output_activation_on_the_acting_forms(out_act):
    """a relu hidden net (h == z for z > 0, exactly) with +1 diagonals and output weights +1 / -1: the head's pre-activation is
    +-relu(obs) exactly, so the mean columns are out_act at both signs of every table magnitude"""
    O, A, hid = sw.ACTING_SHAPE
    alg = acting_engine("relu", out_act)
    e = alg.engine
    template = alg.networks.state_dict()
    obs = sw.sweep_obs(N_ROWS, O)
    single = -(-sw.table().size // O)
    feat = _relu_chain(obs, hid[-1])
    worst, judged = {}, set()
    n_rot = -(-hid[-1] // A)
    for rot in range(2 * n_rot):
        sign = np.float32(1.0 if rot < n_rot else -1.0)
        cols = sw.head_cols(A, hid[-1], rot % n_rot)
        alg.networks.load_state_dict(sw.sweep_state(template, O, head={"policy": sign * sw.one_hot_head(A, hid[-1], rot % n_rot)}, positive=True))
        m = acting_means(e, obs, single)
        assert_batched_forms_agree(m, (out_act, rot))
        z = sign * feat[:, cols]
        want = reference_unique(out_act, z)[0]
        for form, got in m.items():
            r, i = sw.worst(got, want[:got.shape[0]])
            assert r <= 1.0, (form, out_act, rot, r, float(z[:got.shape[0]].reshape(-1)[i]))
            worst[form] = max(worst.get(form, 0.0), r)
        judged |= set(z[:single].reshape(-1).tolist())
    assert set(sw.table().tolist()) <= judged          # (by value: -0 is not reachable through a sum with +0 terms)
    print("edges policy_out %-8s %s" % (out_act, "  ".join("%s %.4f" % kv for kv in sorted(worst.items()))))
    e.close()


@pytest.mark.parametrize("out_act", sw.ACTS)
@pytest.mark.parametrize("path", ["tile", "chain64"])
def test_value_output_activation(path, out_act):
    """column 0 of qout_c0 / qout_c1: q1's output row is +1 on one stored feature of a relu net, q2's is -1 on the same one; the
    feature walks over the observation columns until every table magnitude has been through the head with both signs"""
    O, A, hid, B, _ = sw.UPDATE_SHAPES[path]
    alg, _ = make_pair(O, A, hid, B, value_hidden_activation="relu", policy_hidden_activation="relu", value_output_activation=out_act)
    e = alg.engine
    if path == "tile":
        _tiles(e)
    elif out_act != "gelu":      # (gelu as an output activation is served by the tile-stage kernels at every shape)
        _chains(e)
    template = alg.networks.state_dict()
    worst, judged = 0.0, set()
    for c in range(O):
        row = np.zeros((1, hid[-1]), np.float32)
        row[0, c] = 1.0
        alg.networks.load_state_dict(sw.sweep_state(template, O, head={"q1": row, "q2": -row}, positive=True))
        obs, _ = load_sweep_batch(e, O, A, B)
        e.compute_grads(0)
        e.sync()
        feat = _relu_chain(obs, hid[-1])[:, c]
        for i, sign in ((0, 1.0), (1, -1.0)):
            z = np.float32(sign) * feat
            got = e.debug_read("qout_c%d" % i).reshape(B, 2)[:, 0]
            r, k = sw.worst(got, sw.reference(out_act, z)[0])
            assert r <= 1.0, (path, out_act, c, i, r, float(z[k]))
            worst = max(worst, r)
            judged |= set(z.tolist())
    assert set(sw.table().tolist()) <= judged
    print("edges value_out %-8s %-8s %.4f" % (path, out_act, worst))
    e.close()
