"""The activation epilogue at its breakpoints and tails, on the host: the contract of tests/test_activation_edges_gpu.py.

act_fwd_grad (csrc/dsact_math.h, the scalar form every device path but the packed GELU calls) and the host acting forward
(csrc/dsact_host_act.h: its own vector erf / 2^x, three instruction-set instantiations) over tests/activation_sweep.py's table:
both signs of 0, 2^-120 .. 2^20 and the +-3 ulp neighbourhood of every breakpoint, against a float64 reference written with
numpy / math. The scalar forms hold A QUARTER of the gate (|got - ref| <= 1e-6 + 2e-5 |ref|; worst measured 0.09 of it), so that
what v_exp_f32 and the device libm add on the GPU has the rest. CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import activation_sweep as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def hm():
    import __graft_entry__ as g
    g.build()
    return C.CDLL(os.path.join(ROOT, "oracle", "_build", "libdsact_hostmath.so"))


def p(a):
    return a.ctypes.data_as(FP)


def host_act(lib, act, z):
    z = np.ascontiguousarray(z, np.float32).reshape(-1)
    h, g = np.empty_like(z), np.empty_like(z)
    lib.hm_act.argtypes = [C.c_int, FP, C.c_int, FP, FP]
    lib.hm_act(sw.ACT_ID[act], p(z), z.size, p(h), p(g))
    return h, g


def scalar_report(lib):
    """{(act, "h" | "g"): (worst |got - ref| / gate over the table, z there, the interval that holds it)}"""
    z = sw.table()
    out = {}
    for act in sw.ACTS:
        got = dict(zip("hg", host_act(lib, act, z)))
        ref = dict(zip("hg", sw.reference(act, z)))
        for k in "hg":
            r, i = sw.worst(got[k], ref[k])
            where = [name for name, f in sw.intervals(act) if f(z[i:i + 1])[0]] or ["0"]
            out[(act, k)] = (r, float(z[i]), where[0])
    return out


def test_table_holds_what_the_sweep_needs():
    z = sw.table()
    assert z.size <= sw.TABLE_MAX and z.dtype == np.float32 and np.unique(z.view(np.uint32)).size == z.size
    mag = np.abs(z)
    assert mag.max() == sw.Z_MAX and mag[mag > 0].min() >= np.finfo(np.float32).tiny * 2.0 ** 6      # 2^-120: no denormals
    assert np.array_equal(z[0::2], -z[1::2]) and np.signbit(z[1]) and z[0] == 0 and not np.signbit(z[0])   # both signs, of 0 too
    exps = set(np.frexp(mag[mag > 0])[1] - 1)
    assert set(range(-28, 21)) <= exps and min(exps) == -120
    for b in sw.BREAKPOINTS:             # the breakpoint's float32 and 3 ulp steps to either side, both signs
        v = np.float32(b)
        near = {float(v)}
        lo = hi = v
        for _ in range(sw.ULPS):
            lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
            near |= {float(lo), float(hi)}
        assert len(near) == 2 * sw.ULPS + 1
        for s in (1.0, -1.0):
            assert {s * x for x in near} <= set(z.tolist()), b
    for act in sw.ACTS:
        sw.assert_coverage(act, z, "table")
        h, g = sw.reference(act, z)
        assert np.isfinite(h).all() and np.isfinite(g).all()
    # the smallest case of the GPU test holds every point once
    for name, (O, A, hid, B, _) in sw.UPDATE_SHAPES.items():
        for shift in (0, sw.OBS2_SHIFT):
            z0 = sw.z_layer0(sw.sweep_obs(B, O, shift), min(hid[0], O))
            assert set(z.view(np.uint32).tolist()) <= set(z0.view(np.uint32).reshape(-1).tolist()), name


def test_reference_conventions_at_zero_and_in_the_tails():
    z0 = np.array([0.0, -0.0], np.float32)
    assert sw.reference("relu", z0)[1].tolist() == [0.0, 0.0]
    assert np.allclose(sw.reference("selu", z0)[1], sw.SELU_SCALE * sw.SELU_ALPHA, rtol=1e-15)
    assert sw.reference("elu", z0)[1].tolist() == [1.0, 1.0]
    # against torch in float64 (the modules the reference networks are made of) at a few benign and saturated points
    import torch
    zs = np.array([-30.0, -9.5, -3.0, -0.5, 0.5, 3.0, 9.5, 30.0], np.float32)
    mods = {"gelu": torch.nn.GELU(), "relu": torch.nn.ReLU(), "elu": torch.nn.ELU(), "selu": torch.nn.SELU(),
            "sigmoid": torch.nn.Sigmoid(), "tanh": torch.nn.Tanh()}
    for act, mod in mods.items():
        t = torch.tensor(zs, dtype=torch.float64, requires_grad=True)
        y = mod(t)
        y.sum().backward()
        h, g = sw.reference(act, zs)
        # (torch's float64 GELU is z (1 + erf) / 2: its own cancellation, 1e-16 absolute, is the atol)
        np.testing.assert_allclose(h, y.detach().numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(g, t.grad.numpy(), rtol=1e-12, atol=1e-15)


def test_scalar_forms_hold_a_quarter_of_the_gate(hm):
    rep = scalar_report(hm)
    for (act, k), (r, z, where) in sorted(rep.items()):
        print("host scalar %-8s %s worst err/gate %.4f at z = %.9g (%s)" % (act, k, r, z, where))
    bad = {key: v for key, v in rep.items() if not v[0] <= 0.25}
    assert not bad, bad
    for k in "hg":
        assert rep[("relu", k)][0] == 0.0


def _policy_params(O, A, hid, rot, last_bias=None):
    """flat parameter vector of a policy in arena order (W, b per layer) with the sweep's construction (acting nets: +-1 diagonals,
    or a zero last hidden layer whose bias is the pre-activation) and a one-hot mean head"""
    sizes = [O] + list(hid)
    flat, w_off, b_off, k_in, n_out = [], [], [], [], []
    off = 0
    for l in range(len(hid) + 1):
        bias = None
        if l < len(hid):
            W = sw.hidden_weight(l, sizes[l + 1], sizes[l], O, unit=True)
            if last_bias is not None and l == len(hid) - 1:
                W, bias = np.zeros_like(W), np.asarray(last_bias, np.float32)
        else:
            W = np.zeros((2 * A, sizes[-1]), np.float32)
            W[:A] = sw.one_hot_head(A, sizes[-1], rot)
        w_off.append(off); flat.append(W.reshape(-1)); off += W.size
        b_off.append(off); flat.append(np.zeros(W.shape[0], np.float32) if bias is None else bias); off += W.shape[0]
        k_in.append(W.shape[1]); n_out.append(W.shape[0])
    return np.concatenate(flat), w_off, b_off, k_in, n_out


@pytest.mark.parametrize("act", sw.ACTS)
@pytest.mark.parametrize("O,A,hid", [sw.ACTING_SHAPE, (11, 3, (96, 40))])
def test_host_acting_forward_over_the_table(hm, O, A, hid, act):
    """hm_policy_act on the constructed nets: the mean outputs ARE the last hidden layer's stored features (one-hot head, rotated
    until every feature has been read), held to the float64 reference at the gate -- every instruction set the CPU offers and
    1 / 3 / 4 threads, bitwise equal to each other (every sum has one non-zero addend: no summation order is left).
    Two families of nets: the last hidden layer with zero weights and the table as its bias (its pre-activation is exact: every
    table point is judged), and the observation-driven chain with +-1 diagonals (layer 0 at the table, seen through layer 1)."""
    hm.hm_policy_act.argtypes = [FP, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                 C.c_int, FP, C.c_int, C.c_float, C.c_float, FP, FP, FP, FP, FP, C.c_int, C.c_int, C.POINTER(C.c_int)]
    table = sw.table()
    n = -(-table.size // O)
    obs = sw.sweep_obs(n, O)
    L = len(hid) + 1
    IA, LA = (C.c_int * L), (C.c_longlong * L)
    scale, center = np.ones(A, np.float32), np.zeros(A, np.float32)
    variants = set()

    def means(params, row):
        flat, w_off, b_off, k_in, n_out = params
        per = {}
        for isa, threads in ((0, 1), (1, 1), (2, 1), (-1, 3), (0, 4)):
            logits = np.empty(2 * A, np.float32)
            rc = hm.hm_policy_act(p(flat), L, IA(*k_in), IA(*n_out), LA(*w_off), LA(*b_off), sw.ACT_ID[act], p(row), A, -20.0, 0.5,
                                  None, p(scale), p(center), p(logits), None, isa, threads, None)
            if rc == -2:
                continue                     # this CPU lacks the instruction set
            assert rc >= 0
            per[(isa, threads)] = logits
            variants.add(rc if isa < 0 else isa)
        assert len(per) >= 3
        first = next(iter(per.values()))
        for key, lg in per.items():
            assert np.array_equal(lg.view(np.uint32), first.view(np.uint32)), (act, key)
        assert np.array_equal(first[A:], np.ones(A, np.float32))          # raw log-std 0 -> std 1
        return first[:A]

    worst = {"bias": 0.0, "obs": 0.0}
    judged, seen_cols = set(), set()
    for rot in range(-(-hid[-1] // A)):
        cols = sw.head_cols(A, hid[-1], rot)
        seen_cols |= set(cols.tolist())
        for zb in sw.bias_slices(hid[-1]):
            got = means(_policy_params(O, A, hid, rot, last_bias=zb), obs[rot % n])
            want = sw.reference(act, zb[cols])[0]
            r, i = sw.worst(got, want)
            assert r <= 1.0, ("bias", act, rot, r, float(zb[cols][i]))
            worst["bias"] = max(worst["bias"], r)
            judged |= set(zb[cols].view(np.uint32).tolist())
        ref, z_last = sw.composed_reference(act, obs, hid)
        params = _policy_params(O, A, hid, rot)
        for row in range(n):
            r, i = sw.worst(means(params, obs[row]), ref[row, cols])
            assert r <= 1.0, ("obs", act, rot, row, r, float(z_last[row, cols][i]))
            worst["obs"] = max(worst["obs"], r)
    assert seen_cols == set(range(hid[-1])) and len(variants) >= 2
    assert judged == set(table.view(np.uint32).tolist())
    print("host acting %-8s O=%d %s worst err/gate: exact pre-activation %.4f, through layer 0 %.4f" % (act, O, hid, worst["bias"], worst["obs"]))


@pytest.mark.parametrize("name", list(sw.UPDATE_SHAPES))
def test_deeper_layers_of_every_gpu_case_reach_every_interval(hm, name):
    """The GPU cases assert the coverage of layers l >= 1 on the values they read back; here the same chains are run with the host
    build of the scalar form standing in for the device, so that a construction that cannot meet its coverage fails on a CPU box"""
    O, A, hid, B, acts = sw.UPDATE_SHAPES[name]
    B = min(B, 512)                                    # (the larger batches repeat the same rows)
    for act in acts:
        for shift in (0, sw.OBS2_SHIFT):
            z = sw.z_layer0(sw.sweep_obs(B, O, shift), hid[0])
            for l, w in enumerate(hid):
                if l:
                    z = sw.z_deeper(h.reshape(z.shape[0], -1), w)
                    assert np.isfinite(z).all()
                    sw.assert_coverage(act, z, "%s layer %d shift %d" % (name, l, shift))
                h, g = host_act(hm, act, z)
                assert np.isfinite(h).all() and np.isfinite(g).all()
                for k, got, ref in zip("hg", (h, g), sw.reference(act, z)):
                    r, i = sw.worst(got, ref)
                    assert r <= 0.25, (name, act, l, k, r, float(z.reshape(-1)[i]))
