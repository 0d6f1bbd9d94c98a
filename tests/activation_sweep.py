"""The activation epilogue h = act(z), g = act'(z) at pre-activations that are known exactly (shared by
tests/test_activation_edges_host.py and tests/test_activation_edges_gpu.py). No GPU, no randomness.

Every forward path stores h and g; the backward only multiplies by the stored g. The arithmetic exists in six hand-written
copies (scalar and packed on the device, three vector instantiations on the host), and the parity cases only ever feed it
|z| < 3. This module holds

  table()          the sweep of pre-activations: both signs of 0, of a thinned grid 2^e (1 + m / 16), e = -120 .. 20, and of the
                   +-3 ulp neighbourhood of every breakpoint of the six activations (BREAKPOINTS). |z| <= 2^20, no denormals,
                   at most 550 points: the smallest case (batch 50 x 11 observation columns) holds every point once
  reference()      h and g in float64, written plainly with numpy / math
  GATE             |got - ref| <= 1e-6 + 2e-5 |ref| for h and for g
  intervals()      the pieces of each activation's definition; coverage() counts the points in each
  sweep_state()    nets in which z is exact: layer 0 is one-hot on the observation columns (z0[r, j] = obs[r, j mod O], one product
                   by 1.0 and zero addends), layer l >= 1 is diagonal +-2^k (z_l[r, j] = +-2^k_j h_{l-1}[r, j mod w_{l-1}], exact
                   on the stored h_{l-1}), everything behind is zero weights with benign biases. For forms that expose only
                   their outputs (the acting forwards): a one-hot output layer (one_hot_head), and in front of it either a last
                   hidden layer of zero weights whose BIAS is a slice of the table (bias_slices: z is the bias, exactly) or
                   +-1 diagonals judged against the composed float64 chain (composed_reference)
  sweep_obs()      observation rows that hold the table
"""
import math

import numpy as np

ACT_ID = {"gelu": 0, "relu": 1, "elu": 2, "selu": 3, "sigmoid": 4, "tanh": 5}      # ACT_* of csrc/dsact_math.h
ACTS = tuple(ACT_ID)
SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
SQRT2 = math.sqrt(2.0)
GATE_ABS, GATE_REL = 1e-6, 2e-5
Z_MAX = 2.0 ** 20
TABLE_MAX = 550
# the erf fit's interval split and its clamp (in z = x sqrt 2), 20, expf's overflow, expf(-z)'s underflow, and where ELU / SELU
# and tanh saturate in fp32
BREAKPOINTS = (0.9375 * SQRT2, 4.1 * SQRT2, 20.0, 88.72, 103.97, 17.0, 9.0)
ULPS = 3


def table():
    """float32[T], T <= TABLE_MAX, ordered (+m0, -m0, +m1, -m1, ...) by magnitude"""
    mags = {0.0}
    # the grid, thinned: every 6th exponent below 2^-30 (one mantissa step each, cycling), every exponent from 2^-28 to 2^19
    # with 4 of the 16 mantissa steps (cycling through all 16 over 4 exponents), and 2^20 itself
    for i, e in enumerate(range(-120, -29, 6)):
        mags.add(float(np.float32(2.0 ** e * (1.0 + ((5 * i) % 16) / 16.0))))
    for e in range(-28, 20):
        for q in range(4):
            mags.add(float(np.float32(2.0 ** e * (1.0 + ((4 * q + e) % 16) / 16.0))))
    mags.add(Z_MAX)
    for b in BREAKPOINTS:
        v = np.float32(b)
        lo = hi = v
        mags.add(float(v))
        for _ in range(ULPS):
            lo, hi = np.nextafter(lo, np.float32(0.0)), np.nextafter(hi, np.float32(np.inf))
            mags.add(float(lo)); mags.add(float(hi))
    m = np.array(sorted(mags), np.float32)
    out = np.empty(2 * m.size, np.float32)
    out[0::2], out[1::2] = m, -m
    return out


def _erfc(x):
    return np.vectorize(math.erfc, otypes=[np.float64])(x)


def reference(act, z):
    """(h, g) in float64 of float32 pre-activations z. At z == +-0: relu' = 0, selu' = scale * alpha, elu' = 1 (torch)"""
    z = np.asarray(z, np.float32).astype(np.float64)
    pos = z > 0
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if act == "gelu":
            cdf = 0.5 * _erfc(-z / SQRT2)
            return z * cdf, cdf + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
        if act == "relu":
            return np.where(pos, z, 0.0), pos.astype(np.float64)
        if act == "elu":
            return np.where(pos, z, np.expm1(np.minimum(z, 0.0))), np.where(pos, 1.0, np.exp(np.minimum(z, 0.0)))
        if act == "selu":
            return (SELU_SCALE * np.where(pos, z, SELU_ALPHA * np.expm1(np.minimum(z, 0.0))),
                    np.where(pos, SELU_SCALE, SELU_SCALE * SELU_ALPHA * np.exp(np.minimum(z, 0.0))))
        if act == "sigmoid":
            e = np.exp(-np.abs(z))                       # never overflows
            h = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
            return h, e / ((1.0 + e) * (1.0 + e))        # h (1 - h) without the cancellation of 1 - h
        if act == "tanh":
            h = np.tanh(z)
            return h, 1.0 / np.cosh(np.minimum(np.abs(z), 400.0)) ** 2     # 1 - h^2 without its cancellation
    raise KeyError(act)


def gate(ref):
    return GATE_ABS + GATE_REL * np.abs(np.asarray(ref, np.float64))


def worst(got, ref):
    """max over the elements of |got - ref| / gate, and its position"""
    ref = np.asarray(ref, np.float64).reshape(-1)
    r = np.abs(np.asarray(got, np.float64).reshape(-1) - ref) / gate(ref)
    r = np.where(np.isnan(r), np.inf, r)
    i = int(np.argmax(r))
    return float(r[i]), i


def intervals(act):
    """[(name, mask function of float32 z)]: the pieces of the activation's definition, per sign"""
    neg, posv = (lambda z: np.signbit(z)), (lambda z: ~np.signbit(z))
    if act == "gelu":
        x = lambda z: np.abs(z.astype(np.float64)) / SQRT2
        out = []
        for sname, s in (("+", posv), ("-", neg)):
            out += [(sname + "[0,0.9375]", lambda z, s=s: s(z) & (x(z) <= 0.9375)),
                    (sname + "(0.9375,4.1]", lambda z, s=s: s(z) & (x(z) > 0.9375) & (x(z) <= 4.1)),
                    (sname + ">4.1", lambda z, s=s: s(z) & (x(z) > 4.1))]
        return out
    if act in ("elu", "selu"):
        return [("<-17", lambda z: z < -17), ("(-17,0]", lambda z: (z >= -17) & (z <= 0)), (">0", lambda z: z > 0)]
    if act == "sigmoid":
        return [("<-88", lambda z: z < -88), ("-inside", lambda z: (z >= -88) & (z < 0)), ("+inside", lambda z: (z > 0) & (z <= 88)),
                (">88", lambda z: z > 88)]
    if act == "tanh":
        return [("-<9", lambda z: (z < 0) & (z > -9)), ("+<9", lambda z: (z > 0) & (z < 9)), ("<-9", lambda z: z < -9), (">9", lambda z: z > 9)]
    if act == "relu":
        return [("<0", lambda z: z < 0), (">0", lambda z: z > 0)]
    raise KeyError(act)


def coverage(act, z):
    z = np.asarray(z, np.float32).reshape(-1)
    return {name: int(np.count_nonzero(f(z))) for name, f in intervals(act)}


def assert_coverage(act, z, what, least=2):
    c = coverage(act, z)
    assert all(v >= least for v in c.values()), "%s: %s coverage %s" % (what, act, c)
    return c


# ---- nets with exact pre-activations ------------------------------------------------------------------------------------------
K_CYCLE = (0, 7, 3, 4, 8, 1, 5)        # layer l >= 1, column j: weight +,+,-,-,.. times 2^K_CYCLE[j mod 7] (the table
# alternates in sign, so the sign pattern must not follow the column's parity); 2^7 h reaches 88 from h in (0, 1)


def diag_scale(j, unit=False):
    """unit: +-1 (the acting nets, whose last hidden layer is seen only through the layer behind it)"""
    return (-1.0 if (j >> 1) & 1 else 1.0) * (1.0 if unit else 2.0 ** K_CYCLE[j % len(K_CYCLE)])


def hidden_weight(l, w_out, w_in, O, unit=False, positive=False):
    """float32[w_out, w_in] of hidden layer l (w_in: the stored input width, observation columns first)"""
    W = np.zeros((w_out, w_in), np.float32)
    for j in range(w_out):
        if l == 0:
            W[j, j % O] = 1.0
        else:
            W[j, j % w_in] = 1.0 if positive else diag_scale(j, unit)
    return W


def z_layer0(obs, w_out):
    obs = np.asarray(obs, np.float32)
    return obs[:, np.arange(w_out) % obs.shape[1]]


def z_deeper(h_prev, w_out, unit=False):
    """layer l >= 1 from the STORED output of layer l - 1 (float32; a power of two times a float32 is exact)"""
    h_prev = np.asarray(h_prev, np.float32)
    j = np.arange(w_out)
    s = np.array([diag_scale(int(k), unit) for k in j], np.float32)
    return h_prev[:, j % h_prev.shape[1]] * s[None, :]


def sweep_obs(B, O, shift=0):
    """float32[B, O] holding table()[(i + shift) mod T] at flat position i: every point once where B * O >= T"""
    t = table()
    return t[(np.arange(B * O) + shift) % t.size].reshape(B, O).copy()


Q_BIAS, POLICY_BIAS = (0.25, 0.5), 0.0       # output layers behind the sweep: q = 0.25, raw std = 0.5; policy logits 0


def _layers(sd, net):
    """[(weight key, bias key)] of a net of the state dict, input to output"""
    ws = sorted((k for k in sd if k.startswith(net + ".") and k.endswith(".weight")), key=lambda k: int(k.split(".")[-2]))
    return [(k, k[:-len("weight")] + "bias") for k in ws]


def sweep_state(sd, O, head=None, unit=False, positive=False, last_bias=None):
    """a copy of a state dict of the algorithm's networks (torch tensors) with every net -- online and target -- rebuilt:
    hidden layers exact (hidden_weight, bias 0), output layers zero with benign biases.
    head: {net prefix: float32[rows, w_last]} output weights instead of zeros (acting forms and output activations: one-hot / +-1
          rows; that net's output bias is then 0)
    last_bias: {net prefix: float32[w_last]}: that net's last hidden layer gets ZERO weights and this bias -- its pre-activation
          IS the bias, whatever the layers in front of it hold"""
    import torch

    out = {k: v.detach().cpu().clone() for k, v in sd.items()}
    pick = lambda d, net: next((v for p, v in (d or {}).items() if net.startswith(p)), None)
    for net in sorted({k.split(".")[0] for k in out if k.count(".") >= 2}):
        lay = _layers(out, net)
        for l, (wk, bk) in enumerate(lay):
            w = out[wk]
            if l < len(lay) - 1:
                lb = pick(last_bias, net) if l == len(lay) - 2 else None
                if lb is not None:
                    out[wk] = torch.zeros_like(w)
                    out[bk] = torch.from_numpy(np.asarray(lb, np.float32).copy())
                    assert out[bk].shape == (w.shape[0],)
                else:
                    out[wk] = torch.from_numpy(hidden_weight(l, w.shape[0], w.shape[1], O, unit, positive))
                    out[bk] = torch.zeros_like(out[bk])
            else:
                out[wk] = torch.zeros_like(w)
                b = torch.zeros_like(out[bk])
                hw = pick(head, net)
                if hw is not None:
                    hw = np.asarray(hw, np.float32)
                    out[wk][:hw.shape[0]] = torch.from_numpy(hw.copy())
                elif net.startswith("q"):
                    b[0], b[1] = Q_BIAS
                else:
                    b[:] = POLICY_BIAS
                out[bk] = b
    return out


def one_hot_head(A, w_last, rot):
    """float32[A, w_last]: mean row a reads stored feature (a + rot * A) mod w_last"""
    W = np.zeros((A, w_last), np.float32)
    for a in range(A):
        W[a, (a + rot * A) % w_last] = 1.0
    return W


def head_cols(A, w_last, rot):
    return (np.arange(A) + rot * A) % w_last


def composed_reference(act, obs, hidden, unit=True):
    """(h, z) of the last hidden layer for forms that expose nothing in front of it (the acting forwards): every layer in float64
    from the float32 rounding of the layer before. The form's own h_{l-1} differs from that rounding by its error e, which the
    next layer turns into |s g(z)| e: only nets with |s| = 1 are judged this way (2^8 would carry a tail's absolute error, which
    the gate allows up to 1e-6, far past it)."""
    z = z_layer0(obs, hidden[0])
    for l, w in enumerate(hidden):
        if l:
            z = z_deeper(h.astype(np.float32), w, unit)
        h, g = reference(act, z)
    return h, z


def bias_slices(w_last):
    """[float32[w_last]]: the table cut into biases of the last hidden layer (the last slice wraps around)"""
    t = table()
    return [t[(np.arange(w_last) + s) % t.size].copy() for s in range(0, t.size, w_last)]


# ---- the cases of tests/test_activation_edges_gpu.py (the host contract simulates their deeper layers' coverage) ---------------
# name -> (O, A, hidden, B, activations)
UPDATE_SHAPES = {
    "tile": (11, 3, (96, 40), 50, ACTS),
    "chain64": (24, 6, (64, 64), 64, ACTS),
    "chain128": (24, 6, (128, 128), 64, ("gelu", "selu")),
    "chain256": (24, 6, (256, 256, 256), 64, ("gelu", "selu")),
    "fat_fwd": (11, 6, (128, 128), 512, ACTS),
    "fat16": (24, 6, (256, 256, 256), 1024, ("gelu", "selu")),
    "fat32": (24, 6, (256, 256, 256), 4096, ("gelu", "selu")),
}
ACTING_SHAPE = (32, 32, (64, 64))
OBS2_SHIFT = 7          # obs2 (the target chains' input) holds the table at another offset
