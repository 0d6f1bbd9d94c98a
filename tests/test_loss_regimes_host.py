"""The contract of tests/stress_cases.py, on the oracle alone (no GPU): every stressed case of tests/test_loss_regimes_gpu.py

  * REACHES the regime it is about, at every one of the 3 updates the GPU cases run and for both critics (rows per regime are
    counted from the oracle's intermediates: >= 2 on each side of the clamp and >= 2 inside at update 0, >= 1 later), and
  * is WELL CONDITIONED there: the fp32 oracle against a float64 copy of itself at the same parameters stays inside a quarter
    of every gate the GPU parity cases apply (1e-4 absolute on statistics and the actor loss, 1e-5 relative on the critic
    loss, 3e-5 of scale on the critic gradients), and on the policy gradient inside twice what the unstressed case of the same
    shape and seed shows (a saturated action already costs the unstressed (24, 6) case 5e-5 of scale: helpers.policy_saturation_budget).
    compare_intermediates' absolute gates on the critics' outputs (2e-5) and the actions (2e-6) are held to half.

A kernel that misses a gate on these inputs is wrong; the reference's own rounding cannot be the reason.
"""
import copy

import pytest
import torch

from oracle.dsact_oracle import TB_KEYS
from oracle.dsac_v1_oracle import V1_TB_KEYS
from stress_cases import DIM_ON_MAX, DIM_ON_MIN, EXP_OVERFLOW, V1_CASES, V2_CASES, make_oracle, regime_counts, regime_counts_v1

TILE, CHAIN, HEADLINE = (11, 6, (96, 40), 64), (24, 6, (128, 128), 64), (376, 17, (256, 256, 256), 256)
FAT, FAT4K = (11, 6, (128, 128), 512), (11, 6, (128, 128), 4096)
V2_RUNS = ([(s, c, "TanhGaussDistribution") for s in (TILE, CHAIN, FAT, FAT4K) for c in V2_CASES]
           + [(HEADLINE, c, "TanhGaussDistribution") for c in ("spread", "logstd")]
           + [(s, "logstd", "GaussDistribution") for s in (TILE, CHAIN)])
V1_RUNS = [(s, c) for s in (TILE, CHAIN) for c in V1_CASES]


def to_double(orc):
    """a float64 copy of an oracle at the same parameters (mean_std EMA included)"""
    o = copy.deepcopy(orc)
    for ps in o.p.values():
        for t in ps:
            t.data = t.data.double()
    o.log_alpha.data = o.log_alpha.data.double()
    o.act_high, o.act_low = o.act_high.double(), o.act_low.double()
    for k in ("mean_std1", "mean_std2"):
        if torch.is_tensor(getattr(o, k, None)):
            setattr(o, k, getattr(o, k).double())
    return o


def dbl(d):
    return {k: (v.double() if torch.is_tensor(v) else v) for k, v in d.items()}


def grad_gaps(orc, orc64, nets):
    """max |g32 - g64| / max |g64| per net"""
    out = {}
    for n in nets:
        g32 = torch.cat([t.grad.reshape(-1).double() for t in orc.p[n]])
        g64 = torch.cat([t.grad.reshape(-1) for t in orc64.p[n]])
        out[n] = float((g32 - g64).abs().max() / g64.abs().max())
    return out


def v2_margins(shape, case, dist):
    """[(tb32, counts, gaps)] per update: the oracle's trajectory in fp32, each update also evaluated by its float64 copy"""
    orc, inputs = make_oracle(case, shape, dist)
    rows = []
    for it, (data, noise) in enumerate(inputs):
        o64 = to_double(orc)          # BEFORE the step: compute_gradient moves the mean_std EMA
        tb = orc.compute_gradient(data, noise, keep=True)
        tb64 = o64.compute_gradient(dbl(data), dbl({k: v for k, v in noise.items() if k != "z_discarded"}), keep=True)
        gaps = grad_gaps(orc, o64, ("q1", "q2", "policy"))
        # compare_intermediates' ABSOLUTE gates: 2e-5 on the critics' outputs (the std outputs are the ones the spread case scales)
        # and on the policy mean, 2e-6 on the actions
        gaps["outputs"] = max(float((orc.inter[k].double() - o64.inter[k]).abs().max()) for k in
                              ("q1", "q2", "q1_std", "q2_std", "q1_next", "q2_next", "q1_pi", "q2_pi"))
        gaps["actions"] = max(float((orc.inter[k].double() - o64.inter[k]).abs().max()) for k in ("new_act", "act2"))
        crit = "Loss/Critic loss-RL iter"
        gaps["stats"] = max(abs(tb[k] - tb64[k]) for k in TB_KEYS[:-1] if k != crit)
        gaps["critic_loss"] = abs(tb[crit] - tb64[crit]) / abs(tb64[crit])
        grads = {n: [t.grad.clone() for t in orc.p[n]] for n in ("policy",)}
        rows.append((tb, regime_counts(orc, data, noise), gaps, grads))
        orc.update(it)
    return rows


_BASE = {}


def base_policy_gap(shape, dist, it):
    """the unstressed case of the same shape and seed (computed once per shape); dist "v1": DSAC_V1"""
    key = (shape, dist)
    if key not in _BASE:
        _BASE[key] = [r[1]["policy"] for r in v1_margins(shape, "base")] if dist == "v1" else [r[2]["policy"] for r in v2_margins(shape, "base", dist)]
    return _BASE[key][it]


def check_conditioning(title, it, gaps, base_policy):
    print("%s it%d fp32 vs float64: stats %.1e  critic loss %.1e  grad q %.1e  grad policy %.1e (unstressed %.1e)  q / std outputs %.1e  actions %.1e"
          % (title, it, gaps["stats"], gaps.get("critic_loss", 0.0), max(gaps[k] for k in gaps if k in ("q", "q1", "q2")), gaps["policy"], base_policy,
             gaps.get("outputs", 0.0), gaps.get("actions", 0.0)))
    # (the intermediates' gates are not among the ones the quarter was asked for; half: the kernel's own distance from the exact
    #  value gets the other half. The overflow case's std outputs of ~90 round to 3.8e-6 by themselves.)
    assert gaps.get("outputs", 0.0) <= 0.5 * 2e-5 and gaps.get("actions", 0.0) <= 0.5 * 2e-6, (title, it, gaps)
    assert gaps["stats"] <= 0.25 * 1e-4, (title, it, gaps)
    assert gaps.get("critic_loss", 0.0) <= 0.25 * 1e-5, (title, it, gaps)
    for n in ("q", "q1", "q2"):
        assert gaps.get(n, 0.0) <= 0.25 * 3e-5, (title, it, n, gaps)
    assert gaps["policy"] <= 2.0 * base_policy, (title, it, gaps, base_policy)


def at_least(title, it, name, counts):
    need = 2 if it == 0 else 1
    assert min(counts) >= need, "%s it%d: %s = %s, every entry must be >= %d" % (title, it, name, counts, need)


@pytest.mark.parametrize("shape,case,dist", V2_RUNS, ids=lambda v: str(v).replace(" ", ""))
def test_case_reaches_its_regime_and_is_well_conditioned(shape, case, dist):
    O, A, hid, B = shape
    title = "%s %s%s" % (case, shape, " Gauss" if dist != "TanhGaussDistribution" else "")
    for it, (tb, c, gaps, grads) in enumerate(v2_margins(shape, case, dist)):
        print("%s it%d regimes: %s" % (title, it, c))
        assert c["z"][0] >= 1 and c["z"][1] >= 2 and c["z"][2] >= 1, (title, it, c["z"])     # rows 0-3: 3, -3, 3.5, -4
        if case == "spread":
            for i in (1, 2):
                at_least(title, it, "ratio%d (below 0.1, inside, above 10)" % i, c["ratio%d" % i])
                if shape != HEADLINE:   # (there alpha * logp2 of 17 action dimensions puts nearly every target below q - 3 mean_std)
                    at_least(title, it, "target%d (below -3 ms, inside, above 3 ms)" % i, c["target%d" % i])
        elif case == "threshold":
            for key in ("softplus1", "softplus1_t", "softplus2", "softplus2_t"):       # online and target net
                at_least(title, it, key + " (raw <= 20, > 20)", (c[key][0], c[key][1] + c[key][2]))
        elif case == "overflow":
            for key in ("softplus1", "softplus1_t", "softplus2", "softplus2_t"):
                at_least(title, it, key + " (20 < raw <= 88.73, raw > 88.73)", c[key][1:])
        elif case == "reward":
            for i in (1, 2):
                at_least(title, it, "huber%d (d < -50, quadratic, d > 50)" % i, c["huber%d" % i])
        elif case == "logstd":
            at_least(title, it, "logstd (below, inside, above)", c["logstd"])
            at_least(title, it, "target policy's std on (lower, upper) bound", c["logstd_t"])
            if it == 0:     # the bias moves with the first update: exactly ON the bound at update 0 only
                assert c["logstd_on"] == (B, B), (title, c)
                # torch's clamp passes the gradient ON its bounds (min <= x <= max): a gate with > / < would zero these two
                gb = grads["policy"][-1]
                assert gb[A + DIM_ON_MAX] != 0 and gb[A + DIM_ON_MIN] != 0, (title, gb)
        elif case == "twin":
            assert c["tie_next"] == B and c["tie_pi"] == B, (title, it, c)
        check_conditioning(title, it, gaps, base_policy_gap(shape, dist, it))


def v1_margins(shape, case):
    orc, inputs = make_oracle(case, shape, v1=True)
    rows = []
    for it, (data, noise) in enumerate(inputs):
        o64 = to_double(orc)
        counts = regime_counts_v1(orc, data, noise)
        tb = orc.compute_gradient(data, noise)
        tb64 = o64.compute_gradient(dbl(data), dbl({k: v for k, v in noise.items() if k != "z_discarded"}))
        gaps = grad_gaps(orc, o64, ("q", "policy"))
        gaps["stats"] = max(abs(tb[k] - tb64[k]) for k in V1_TB_KEYS[:-1])
        rows.append((counts, gaps, orc.p["policy"][-1].grad.clone()))
        orc.update(it)
    return rows


@pytest.mark.parametrize("shape,case", V1_RUNS, ids=lambda v: str(v).replace(" ", ""))
def test_v1_case_reaches_its_regime_and_is_well_conditioned(shape, case):
    O, A, hid, B = shape
    title = "v1 %s %s" % (case, shape)
    for it, (c, gaps, gb) in enumerate(v1_margins(shape, case)):
        print("%s it%d regimes: %s" % (title, it, c))
        assert c["z"][0] >= 1 and c["z"][1] >= 2 and c["z"][2] >= 1, (title, it, c["z"])
        if case == "logstd":
            at_least(title, it, "logstd (below, inside, above)", c["logstd"])
            if it == 0:
                assert c["logstd_on"] == (B, B), (title, c)
                assert gb[A + DIM_ON_MAX] != 0 and gb[A + DIM_ON_MIN] != 0, (title, gb)
        else:
            at_least(title, it, "td (below -TD_bound, inside, above TD_bound)", c["td"])
        check_conditioning(title, it, gaps, base_policy_gap(shape, "v1", it))


def test_exp_overflow_constant():
    """above EXP_OVERFLOW a softplus that lost its threshold gives inf (and its derivative inf / inf); just below, it is exact"""
    x = torch.tensor([EXP_OVERFLOW], dtype=torch.float32)
    assert torch.isinf(torch.exp(x)).all() and torch.isfinite(torch.exp(x - 0.02)).all()
    assert torch.log1p(torch.exp(x - 0.02)) == x - 0.02
