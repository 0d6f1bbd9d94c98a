"""Stress cases for the per-sample glue of the loss (shared by tests/test_loss_regimes_host.py and _gpu.py).

The benign parity inputs (freshly initialised nets, N(0,1) rewards) never reach the variance-ratio clamp, the linear part of the
Huber loss, a critic std output above softplus' threshold, the log-std clamp or a tie of the twin critics. Each case below
changes ONE thing of the default initialisation (or of the minibatch) so that one of those regimes is populated on both sides
and inside, and stays well conditioned: tests/test_loss_regimes_host.py is the contract (coverage counts per step, and the
oracle in fp32 against itself in float64 inside a quarter of every parity gate) that holds before any GPU case runs.

  spread   the std row of every critic's output layer scaled by KS (+ KB on its bias), per shape and critic: the variance ratio
           clamped at 0.1 and at 10 and inside, both sides of the +-3 mean_std target clamp. KS stays <= 80 (200 at the headline
           shape): the scale multiplies the rounding of the row's dot product, and the std outputs are gated at 2e-5 ABSOLUTE
  threshold / overflow   the same row x 30 with the bias carrying the size (exact): raw std outputs on both sides of softplus'
           threshold of 20 / of 88.73, where exp overflows in fp32 -- the only place a softplus WITHOUT its threshold differs
           from one with it (log1p(exp(x)) == x to the last bit below)
  reward   rewards x RF: both signs of the Huber loss' linear part (|q - target| > 50) next to its quadratic part
  logstd   log-std bounds (-2, 0) with one action dimension exactly ON each bound (zero weight row: the raw value IS the bias,
           bit for bit in any summation order), one beyond each, the rest inside
  twin     q2 := q1 (online and target): every row ties in min(q1', q2') / where(q1' < q2', ..) and in the actor's min
  td       (DSAC_V1) rewards x RF_V1 against TD_bound: both sides and the inside of the fixed clamp; also with bound=False
Every case puts rows 0-3 of z5 / z6 (V1: z_t) on and beyond the +-3 clamp.
"""
import numpy as np
import torch

from helpers import synth_batch
from oracle.dsact_oracle import DsactOracle, default_config, draw_noise
from oracle.dsac_v1_oracle import DsacV1Oracle, draw_noise_v1

ACT_LIMIT, P_DONE, STEPS = 0.4, 0.1, 3
Z_EDGE = (3.0, -3.0, 3.5, -4.0)
LOGSTD_BOUNDS = (-2.0, 0.0)
LOGSTD_KW = dict(policy_min_log_std=LOGSTD_BOUNDS[0], policy_max_log_std=LOGSTD_BOUNDS[1])
# action dimensions of the logstd case: exactly on the upper bound, above it, exactly on the lower bound, below it
DIM_ON_MAX, DIM_ABOVE, DIM_ON_MIN, DIM_BELOW = 0, 1, 2, 3
RF, RF_V1, TD_BOUND_V1 = 60.0, 10.0, 10.0
EXP_OVERFLOW = 88.73          # expf(x) == inf in fp32 above 88.7228

# (O, A, hidden, B) -> (KS, KB): tuned on the CPU oracle per shape (tests/test_loss_regimes_host.py asserts the counts)
SPREAD = {     # ((KS, KB) of q1 / q1_target, (KS, KB) of q2 / q2_target)
    (11, 6, (96, 40), 64): ((80.0, 3.0), (65.0, -4.0)),
    (24, 6, (128, 128), 64): ((65.0, 2.0), (65.0, -3.0)),
    (376, 17, (256, 256, 256), 256): ((200.0, 0.0), (200.0, 0.0)),
    (11, 6, (128, 128), 512): ((80.0, -3.0), (65.0, 0.0)),
    (11, 6, (128, 128), 4096): ((50.0, -2.0), (65.0, 0.0)),
}

# every shape, both critics: raw std outputs within ~5 of softplus' threshold / of exp's overflow, on both sides
THRESHOLD, OVERFLOW = (30.0, 20.0), (30.0, 88.7)

V2_CASES = ("spread", "threshold", "overflow", "reward", "logstd", "twin")
V1_CASES = ("logstd", "td", "td_unbounded")


def _out_layer(sd, net):
    """key stem of net's output layer ("q1.q.4" ...): the Linear with the highest index"""
    idx = max(int(k.split(".")[2]) for k in sd if k.startswith(net + ".") and k.endswith(".weight"))
    sub = [k.split(".")[1] for k in sd if k.startswith(net + ".") and k.endswith(".weight")][0]
    return "%s.%s.%d" % (net, sub, idx)


def stress_state(case, sd, shape=None):
    """a modified copy of a state dict of the algorithm's networks (DSAC_V2's or DSAC_V1's, the HIP container's or the oracle's)"""
    sd = {k: v.detach().cpu().clone() for k, v in sd.items()}
    nets = sorted({k.split(".")[0] for k in sd if "." in k})
    for c in case.split("+"):
        if c in ("spread", "threshold", "overflow"):
            for net in nets:
                if net.startswith("q"):
                    ks, kb = {"threshold": THRESHOLD, "overflow": OVERFLOW}.get(c) or SPREAD[shape][1 if net.startswith("q2") else 0]
                    stem = _out_layer(sd, net)
                    sd[stem + ".weight"][1] *= ks
                    sd[stem + ".bias"][1] += kb
        elif c == "logstd":
            for net in nets:
                if net.startswith("policy"):
                    stem = _out_layer(sd, net)
                    w, b = sd[stem + ".weight"], sd[stem + ".bias"]
                    A = b.numel() // 2
                    assert A >= 5
                    b[A:] -= 1.0                                   # the rest: inside
                    w[A + DIM_ON_MAX] = 0.0; b[A + DIM_ON_MAX] = LOGSTD_BOUNDS[1]
                    b[A + DIM_ABOVE] += 1.0 + 1.5
                    w[A + DIM_ON_MIN] = 0.0; b[A + DIM_ON_MIN] = LOGSTD_BOUNDS[0]
                    b[A + DIM_BELOW] += 1.0 - 4.0
        elif c == "twin":
            for k in list(sd):
                if k.startswith("q1.") or k.startswith("q1_target."):
                    sd["q2" + k[2:]] = sd[k].clone()
        else:
            assert c in ("base", "reward", "td", "td_unbounded"), c
    return sd


def stress_inputs(case, O, A, B, steps=STEPS, v1=False, seed=5):
    """[(data, noise)] of `steps` updates: synth_batch / the reference's noise draws, then the case's change of the minibatch"""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(steps):
        data = synth_batch(rng, B, O, A, lim=ACT_LIMIT, p_done=P_DONE)
        torch.manual_seed(1000 + it)
        noise = draw_noise_v1(B, A) if v1 else draw_noise(B, A)
        if case != "base":
            for k in (("z_t",) if v1 else ("z5", "z6")):
                noise[k][:4] = torch.tensor(Z_EDGE)
        for c in case.split("+"):
            if c == "reward":
                data["rew"] = data["rew"] * RF
            elif c in ("td", "td_unbounded"):
                data["rew"] = data["rew"] * RF_V1
        out.append((data, noise))
    return out


def case_kwargs(case, v1=False):
    kw = {}
    for c in case.split("+"):
        if c == "logstd":
            kw.update(LOGSTD_KW)
        if c == "td_unbounded":
            kw["bound"] = False
    if v1:
        kw["td_bound"] = TD_BOUND_V1
    return kw


def make_oracle(case, shape, dist="TanhGaussDistribution", v1=False):
    """(oracle at the stressed default initialisation under torch.manual_seed(0), [(data, noise)] of the STEPS updates): what the
    host contract evaluates and what the GPU cases load (init=orc.state_dict()) and feed (prepare_hook)"""
    O, A, hid, B = shape
    kw = case_kwargs(case, v1)
    lim = {k[len("policy_"):]: v for k, v in kw.items() if k.startswith("policy_")}
    if v1:
        cfg = default_config(O, A, hid, act_limit=ACT_LIMIT, TD_bound=kw["td_bound"], bound=kw.get("bound", True), **lim)
    else:
        cfg = default_config(O, A, hid, act_limit=ACT_LIMIT, act_dist=dist, **lim)
    torch.manual_seed(0)
    orc = (DsacV1Oracle if v1 else DsactOracle)(cfg)
    orc.load_state_dict(stress_state(case, orc.state_dict(), shape))
    return orc, stress_inputs(case, O, A, B, v1=v1)


def prepare_hook(inputs):
    """run_case's `prepare(it, data, noise)`: the precomputed stressed inputs of update `it`"""
    return lambda it, data, noise: inputs[it]


# ---- which rows reach which regime (from the oracle's intermediates of the step just evaluated, BEFORE its update) ---------
def _three(x, lo, hi):
    return (int((x < lo).sum()), int(((x >= lo) & (x <= hi)).sum()), int((x > hi).sum()))


def regime_counts(orc, data, noise):
    """DsactOracle after compute_gradient(keep=True): rows per regime, per critic where there are two"""
    I, cfg = orc.inter, orc.cfg
    A = cfg["act_dim"]
    alpha = orc._alpha()
    c = {}
    z5, z6 = (torch.clamp(noise[k].to(I["q1"].dtype), -3, 3) for k in ("z5", "z6"))
    pick1 = I["q1_next"] < I["q2_next"]
    qns = torch.where(pick1, I["q1_next"] + z5 * I["q1n_std"], I["q2_next"] + z6 * I["q2n_std"])
    tqs = data["rew"] + (1 - data["done"]) * cfg["gamma"] * (qns - alpha * I["log_prob_act2"])
    for i, ms in ((1, orc.mean_std1), (2, orc.mean_std2)):
        q, std = I["q%d" % i], I["q%d_std" % i]
        c["ratio%d" % i] = _three(ms ** 2 / (std ** 2 + 0.1), 0.1, 10.0)              # (below 0.1, inside, above 10)
        c["huber%d" % i] = _three(q - I["target_q%d" % i], -50.0, 50.0)               # (d < -50, quadratic, d > 50)
        c["target%d" % i] = _three(tqs - q, -3 * float(ms), 3 * float(ms))            # +-3 mean_std clamp of the bounded target
        raw, raw_t = I["z_q%d" % i][-1][:, 1], I["q%dn_std" % i]
        for key, x in (("softplus%d" % i, raw), ("softplus%d_t" % i, raw_t)):        # (target net: softplus(x) > 20 <=> x > 20)
            c[key] = (int((x <= 20).sum()), int(((x > 20) & (x <= EXP_OVERFLOW)).sum()), int((x > EXP_OVERFLOW).sum()))
    ls = I["z_pi"][-1][:, A:]
    lo, hi = cfg["min_log_std"], cfg["max_log_std"]
    c["logstd"] = _three(ls, lo, hi)[:1] + (int(((ls > lo) & (ls < hi)).sum()),) + _three(ls, lo, hi)[2:]   # (below, strictly inside, above)
    c["logstd_on"] = (int((ls == lo).sum()), int((ls == hi).sum()))
    std_t = I["logits_2"][:, A:]
    c["logstd_t"] = (int((std_t == float(np.exp(np.float32(lo)))).sum()), int((std_t == float(np.exp(np.float32(hi)))).sum()))
    c["tie_next"] = int((I["q1_next"] == I["q2_next"]).sum())
    c["tie_pi"] = int((I["q1_pi"] == I["q2_pi"]).sum())
    used = torch.where(pick1, noise["z5"], noise["z6"])
    c["z"] = (int((used < -3).sum()), int((used.abs() == 3).sum()), int((used > 3).sum()))
    return c


def regime_counts_v1(orc, data, noise):
    """DsacV1Oracle (it keeps no intermediates): the forward restated with its own functions at the current parameters"""
    from oracle.dsact_oracle import mlp_forward, tanh_gauss_rsample

    cfg, A = orc.cfg, orc.cfg["act_dim"]
    with torch.no_grad():
        logits_2 = orc._pi(data["obs2"], orc.p["policy_target"])
        act2, lp2 = tanh_gauss_rsample(logits_2, noise["eps_2"], orc.act_high, orc.act_low)
        q, _ = orc._q(data["obs"], data["act"], orc.p["q"])
        qn, qn_std = orc._q(data["obs2"], act2, orc.p["q_target"])
        tq = data["rew"] + (1 - data["done"]) * cfg["gamma"] * (qn + torch.clamp(noise["z_t"], -3, 3) * qn_std - orc._alpha() * lp2)
        ls = mlp_forward(data["obs"], orc.p["policy"], None, cfg.get("policy_act", "gelu"))[:, A:]     # raw log-std (before its clamp)
    lo, hi = cfg["min_log_std"], cfg["max_log_std"]
    c = {"td": _three(tq - q, -orc.TD_bound, orc.TD_bound)}
    c["logstd"] = (int((ls < lo).sum()), int(((ls > lo) & (ls < hi)).sum()), int((ls > hi).sum()))
    c["logstd_on"] = (int((ls == lo).sum()), int((ls == hi).sum()))
    c["z"] = (int((noise["z_t"] < -3).sum()), int((noise["z_t"].abs() == 3).sum()), int((noise["z_t"] > 3).sum()))
    return c
