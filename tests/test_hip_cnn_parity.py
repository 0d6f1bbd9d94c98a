"""Parity of the HIP path with the CNN approximators (BASELINE.json
configs[3]) against the CNN oracle (oracle/dsact_oracle_cnn.py, pinned bit-exact to the live reference)
and against the reference digests in tests/golden/step_cnn_type2.npz.

Gates as in test_hip_parity.py: tb_info within 1e-4 absolute (critic loss 1e-5 relative); gradients relative to each
tensor's scale, with the ReLU-kink elements located, verified to be kinks and budgeted; parameters within 1e-5 of the
oracle for every element except the enumerated ill-conditioned ones, which must be explained by their own measured
gradient difference through Adam (AdamNoise); gathered replay rows bit-exact.
"""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, hip_kwargs
from oracle.dsact_oracle import TB_KEYS, draw_noise
from oracle.dsact_oracle_cnn import conv_out_hw, DsactCnnOracle, cnn_config, conv_forward, synth_image_batch
from test_hip_parity import AdamNoise, Report

pytestmark = pytest.mark.gpu


def cnn_kwargs(obs_shape, A, conv_type, B, **over):
    kw = hip_kwargs(tuple(obs_shape), A, (256, 256, 256), B, act_limit=1.0, **over)
    for key in ("value", "policy"):
        kw[key + "_func_type"] = "CNN"
        kw[key + "_conv_type"] = conv_type
        kw.pop(key + "_hidden_sizes")
    return kw


def make_pair(obs_shape, A, conv_type, B, seed=0, **over):
    from dsac_v2_hip import DSAC_V2_HIP

    torch.manual_seed(seed)
    alg = DSAC_V2_HIP(**cnn_kwargs(obs_shape, A, conv_type, B, strict_rng=True, **over))
    cfg = cnn_config(obs_shape, A, conv_type)
    orc = DsactCnnOracle(cfg, state_dict={k: v.cpu() for k, v in alg.networks.state_dict().items()})
    return alg, orc, cfg


def np_of(t):
    return t.detach().cpu().contiguous().numpy()


def run_case(title, obs_shape, A, conv_type, B, steps, golden=None, chains=None, device_noise=None):
    """device_noise: a Philox key. The update runs in its default mode (strict_rng=False): the noise is drawn in the kernels
    (set_device_rng once, never set_noise), read back after compute_grads, held to tests/noise_reference.py, and handed to the
    oracle as that step's noise bit for bit -- everything below it is compared as with uploaded noise, at the same gates."""
    rep = Report(title)
    alg, orc, cfg = make_pair(obs_shape, A, conv_type, B)
    e = alg.engine
    if chains is not None:   # the twin MLP trunks over the conv features as row-slice chain units (batch % 16 == 0, equal widths)
        assert e.chain_active == chains
    if device_noise is not None:
        from test_update_noise_gpu import read_device_noise
        e.set_device_rng(device_noise)
    names = {n: orc._names(n) for n in ("q1", "q2", "policy")}
    orc.keep_conv = True
    lrs = {"q1": orc.cfg["lr_q"], "q2": orc.cfg["lr_q"], "policy": orc.cfg["lr_pi"]}
    adam_noise = {name: AdamNoise([(net, p.numel(), lrs[net])]) for net in names for name, p in zip(names[net], orc.p[net])}
    n_kinks = 0
    n_digest_rows = 0
    for it in range(steps):
        data = synth_image_batch(cfg, B, seed=it)
        torch.manual_seed(1000 + it)
        noise = draw_noise(B, A)
        e.load_batch(*(data[k].numpy() for k in ("obs", "act", "rew", "obs2", "done")))
        if device_noise is None:
            e.set_noise(noise["eps_new"].numpy(), noise["eps_2"].numpy(), noise["z5"].numpy(), noise["z6"].numpy())
        e.compute_grads(it)
        e.sync()
        if device_noise is not None:
            noise = {k: torch.from_numpy(v) for k, v in read_device_noise(e, device_noise, it).items()}
        # ReLU kinks. A pre-activation within rounding noise of 0 lands on either side of the ReLU depending on the
        # summation order, and the gradient is discontinuous there (the whole upstream gradient of that pixel appears or
        # disappears) -- both choices are valid subgradients. The reference is therefore evaluated with the ReLU decisions
        # the HIP kernels made on the same images (oracle conv_forward(masks=...)): identical wherever the two agree,
        # HIP's choice where they do not, and every such element must BE a kink (|z| < 1e-5 in the reference's own
        # arithmetic). No tolerance below is widened for it, in this or any later iteration.
        C_, H_, W_ = cfg["obs_dim"]
        dims = conv_out_hw(H_, W_, orc.ks, orc.st)
        orc.relu_masks, orc.mask_input, orc.kinks = {}, data["obs"], []
        hip_act = {}
        for st_, net in enumerate(("q1", "q2", "policy")):
            ms = []
            for j, (oh, ow) in enumerate(dims):
                a = e.debug_read("cact.%d.%d" % (st_, j))
                hip_act[(net, j)] = a
                ms.append(torch.as_tensor(a.reshape(B, oh, ow, orc.ch[j]) > 0).permute(0, 3, 1, 2).contiguous())
            orc.relu_masks[net] = ms
        orc.conv_acts = []
        tb_ref = orc.compute_gradient(data, noise, keep=(it == 0))
        for net, j, cnt, zmax in orc.kinks:
            assert zmax < 1e-5, "ReLU decisions differ at a pre-activation of %g (%s conv %d): not a kink" % (zmax, net, j)
            n_kinks += cnt
        if it == 0:
            # conv features of q1(obs) sit in the observation columns of the q1(obs, act) input rows
            F = e.layout.feat_dim
            ld = e.debug_read("X0").size // B
            conv, _, _ = orc._split(orc.p["q1"])
            with torch.no_grad():
                feat = conv_forward(data["obs"], conv, orc.st)
            rep.cmp("features q1(obs)", e.debug_read("X0").reshape(B, ld)[:, :F], feat, 1e-5, 1e-5)
            rep.cmp("new_act", e.debug_read("XP").reshape(B, ld)[:, F:F + A], orc.inter["new_act"], 5e-6)
            rep.cmp("q1", e.debug_read("qout_c0").reshape(B, 2)[:, 0], orc.inter["q1"], 5e-5)
            rep.cmp("q1_pi", e.debug_read("qout_p0").reshape(B, 2)[:, 0], orc.inter["q1_pi"], 5e-5)
            rep.cmp("d_new_act", e.debug_read("d_new_act"), orc.inter["d_new_act"], 1e-9, 3e-4)
        first = {}
        for net, acts in orc.conv_acts:
            first.setdefault(net, acts)     # first call of each online net: (obs) with gradients
        for net in ("q1", "q2", "policy"):
            for j, a in enumerate(first[net]):
                ref = a.detach().permute(0, 2, 3, 1).reshape(-1).numpy()
                rep.cmp("it%d act %s.conv.%d" % (it, net, 2 * j), hip_act[(net, j)], ref, 1e-5, 1e-5)
        gv = alg._grad_views()
        for net in ("q1", "q2", "policy"):
            for name, g_hip, p_ref in zip(names[net], gv[net], orc.p[net]):
                rep.cmp("it%d grad %s" % (it, name), np_of(g_hip), p_ref.grad, 1e-9, 5e-4)
        rep.cmp("it%d grad log_alpha" % it, [float(gv["log_alpha"])], [float(orc.log_alpha.grad)], 1e-6, 1e-5)
        delayed = it % orc.cfg["delay_update"] == 0
        for net in ("q1", "q2", "policy"):
            if net == "policy" and not delayed:
                continue
            for name, g_hip, p_ref in zip(names[net], gv[net], orc.p[net]):
                adam_noise[name].step(np_of(p_ref.grad).reshape(-1), np_of(g_hip).reshape(-1), (net,))
        e.apply_update(it)
        orc.update(it)
        st = e.read_stats()
        for k in TB_KEYS[:-1]:
            if k.startswith("Loss/Critic"):
                rep.cmp("it%d %s" % (it, k.split("/")[-1][:18]), [st[k]], [float(tb_ref[k])], 1e-6, 1e-5)
            else:
                rep.cmp("it%d %s" % (it, k.split("/")[-1][:18]), [st[k]], [float(tb_ref[k])], 1e-4)
        if golden is not None:
            crit = TB_KEYS.index("Loss/Critic loss-RL iter")
            keep_i = [i for i in range(len(TB_KEYS) - 1) if i != crit]
            tb_g = np.asarray(golden["s%d/tb" % it], np.float64)
            rep.cmp("it%d tb vs reference" % it, [st[TB_KEYS[i]] for i in keep_i], tb_g[keep_i], 1e-4)
            rep.cmp("it%d critic loss vs reference" % it, [st[TB_KEYS[crit]]], [tb_g[crit]], 1e-6, 1e-5)
        sd, osd = alg.networks.state_dict(), orc.state_dict()
        assert list(sd.keys()) == list(osd.keys())
        # every element within 1e-5, except elements whose own measured gradient difference (summation order, a ReLU
        # kink upstream) explains more through Adam's division by sqrt(v_hat) -- enumerated per tensor
        got_all, want_all, bound_all, lr_steps = [], [], [], 0.0
        worst_t = 0.0
        for k in sd:
            if "_target" in k:
                worst_t = max(worst_t, float((sd[k].cpu() - osd[k]).abs().max()))
            elif k in adam_noise:
                got_all.append(np_of(sd[k]).reshape(-1))
                want_all.append(np_of(osd[k]).reshape(-1))
                bound_all.append(adam_noise[k].bound)
                lr_steps = max(lr_steps, adam_noise[k].lr_steps)
        rep.cmp_params("it%d params" % it, np.concatenate(got_all), np.concatenate(want_all), np.concatenate(bound_all), 1e-5,
                       lr_steps)
        rep.cmp("it%d targets (max over tensors)" % it, [worst_t], [0.0], 2e-6)
        if golden is not None and n_kinks == 0:
            # per-tensor parameter sums against the UNMODIFIED reference's digest. Budget per tensor, enumerated: what its
            # elements may differ by (1e-6 rounding each, adding up like a random walk: 3 sqrt(N) 1e-6, plus each element's
            # own Adam noise bound from the measured gradient difference) + the fp32 rounding of the sum itself. (After a
            # verified ReLU kink the reference's digest took the other subgradient: HIP is then compared with the oracle
            # only -- above, at unchanged tolerances.)
            keys = list(sd.keys())
            sums = np.array([float(v.double().sum()) for v in sd.values()])
            want = np.asarray(golden["s%d/param_sums" % it], np.float64)
            tol = np.array([1e-6 * abs(w_) + 3e-6 * np.sqrt(sd[k].numel()) + (float(adam_noise[k].bound.sum()) if k in adam_noise else 0.0)
                            for k, w_ in zip(keys, want)])
            rep.cmp_each("it%d param sums vs reference" % it, sums, want, tol)
            n_digest_rows += 1
        elif golden is not None:
            # (visible in the report: the digest row was NOT checked on this iteration and why)
            rep.rows.append(("it%d param sums vs reference: SKIPPED after %d verified ReLU kink(s)" % (it, n_kinks), 0.0, 0.0, 0.0, True))
    # structural zeros of the twin output layers stay exactly zero (include/dsact.h)
    lay = e.layout
    mask = torch.ones(lay.n_online, dtype=torch.bool)
    for net in ("q1", "q2", "policy"):
        for _, _, off, shape, strides in lay.param_views(net):
            idx = torch.as_strided(torch.arange(lay.n_online), shape, strides, off).reshape(-1)
            mask[idx] = False
    mask[lay.log_alpha_offset] = False
    assert int(mask.sum()) > 0
    assert float(e.online.cpu()[mask].abs().max()) == 0.0
    assert float(e.adam_m.cpu()[mask].abs().max()) == 0.0
    assert e.get_state()["adam_steps"][0] == steps
    if golden is not None:
        # on the COMMITTED seed no pre-activation sits within rounding noise of a ReLU kink (profiles/
        # r04_final_parity_report.txt: 0 kinks, every digest row checked), so every iteration's parameter sums must have
        # been compared with the unmodified reference's digest. A kernel change that moves a pre-activation across 0 on this
        # seed shows up HERE instead of silently dropping the only rows that tie the CNN path to the reference itself
        # (regenerate the fixture on another seed with oracle/make_golden.py if that ever happens legitimately).
        assert n_kinks == 0 and n_digest_rows == steps, (
            "reference-digest rows checked on %d of %d iterations (%d ReLU kink(s)) on the committed seed" % (n_digest_rows, steps, n_kinks))
    rep.finish()


def test_cnn_type2_vs_oracle_and_reference_golden():
    z = np.load(os.path.join(GOLDEN, "step_cnn_type2.npz"))
    run_case("cnn type_2 (3,96,96) B=8", tuple(int(v) for v in z["cfg_obs_shape"]), int(z["cfg_act_dim"]),
             str(z["cfg_conv_type"]), int(z["cfg_batch"]), int(z["cfg_steps"]), golden=z)


def test_cnn_type1():
    run_case("cnn type_1 (4,84,84) B=4", (4, 84, 84), 2, "type_1", 4, steps=2)


def test_cnn_type2_b256():
    """BASELINE.json configs[3] at its full batch: conv stacks + the twin trunks on the row-slice chains."""
    run_case("cnn type_2 (3,96,96) B=256", (3, 96, 96), 3, "type_2", 256, steps=2, chains=True)


def test_cnn_type2_b16_twin_trunk_chains():
    """smallest batch the chain kernels take: several updates, so the fused Adam / Polyak of the twin-trunk weight-gradient
    tiles (dense first layer, per-trunk hidden blocks, block-diagonal output layer) feeds the next forward passes."""
    run_case("cnn type_2 (3,96,96) B=16 (twin trunks on the chains)", (3, 96, 96), 3, "type_2", 16, steps=4, chains=True)


def test_cnn_type2_b16_default_mode_update_against_the_oracle():
    """strict_rng=False: the kernels' own draws (Philox streams 1 .. 3, tests/noise_reference.py) read back and fed to the CNN
    oracle bit for bit -- activations, gradients, statistics and parameters at the gates of the uploaded-noise cases"""
    run_case("cnn type_2 (3,96,96) B=16 device noise", (3, 96, 96), 3, "type_2", 16, steps=2, chains=True, device_noise=0x5DEECE66D1234567)


def test_cnn_type2_b16_tile_path_switch(monkeypatch):
    """DSACT_NO_CHAIN_CNN keeps the twin trunks on the stage tiles (the round-1 path, the fallback)."""
    monkeypatch.setenv("DSACT_NO_CHAIN_CNN", "1")
    run_case("cnn type_2 (3,96,96) B=16 (tile path)", (3, 96, 96), 3, "type_2", 16, steps=2, chains=False)


def test_cnn_type2_b512_large_batch_paths():
    """batch 512: the twin trunks run 8-row chain slices (one gradient arena up to batch 1024) while the conv stacks keep
    their own chunked weight gradient."""
    run_case("cnn type_2 (3,96,96) B=512", (3, 96, 96), 3, "type_2", 512, steps=1, chains=True)


@pytest.mark.parametrize("B,steps", [(16, 4), (512, 2)])
def test_cnn_fused_step_equals_split_path(B, steps):
    """fused step (Adam / Polyak inside the weight-gradient tiles and the conv reduce) == gradient halves + streaming Adam,
    bit for bit, on the chain path of the twin trunks."""
    a1, _, cfg = make_pair((3, 96, 96), 3, "type_2", B, seed=3)
    a2, _, _ = make_pair((3, 96, 96), 3, "type_2", B, seed=3)
    for it in range(steps):
        d = synth_image_batch(cfg, B, seed=10 + it)
        torch.manual_seed(50 + it)
        a1.local_update(d, it)                       # fused step
        torch.manual_seed(50 + it)
        _, info = a2.get_remote_update_info(d, it)   # gradients, then the streaming Adam kernel
        a2.remote_update(info)
    s1, s2 = a1.networks.state_dict(), a2.networks.state_dict()
    for k in s1:
        assert torch.equal(s1[k].cpu(), s2[k].cpu()), k


@pytest.mark.parametrize("B", [16, 256])
def test_cnn_identity_col2im_layer_fused_equals_dcol_plus_col2im(B, monkeypatch):
    """type_2's last conv layer has one output pixel and a kernel as large as its input: col2im is the identity there, and round 6
    applies the ReLU mask in the dCol product's epilogue, straight into the previous layer's dY (csrc/dsact_kernels.h
    MULG_RELU_MASK). Against the two-launch form (DSACT_NO_DCOL_IDENT) every parameter must agree bit for bit."""
    nets = []
    for two_launch in (False, True):
        if two_launch:
            monkeypatch.setenv("DSACT_NO_DCOL_IDENT", "1")
        a, _, cfg = make_pair((3, 96, 96), 3, "type_2", B, seed=3)
        monkeypatch.delenv("DSACT_NO_DCOL_IDENT", raising=False)
        for it in range(3):
            d = synth_image_batch(cfg, B, seed=10 + it)
            torch.manual_seed(50 + it)
            a.local_update(d, it)
        assert a.engine.debug_get("dcol_ident") == (0.0 if two_launch else 1.0)
        nets.append(a.networks.state_dict())
    for k in nets[0]:
        assert torch.equal(nets[0][k].cpu(), nets[1][k].cpu()), k


def test_cnn_replay_rows_bit_exact_and_policy_forward():
    from training.hip_replay_buffer import HipReplayBuffer

    obs_shape, A, B = (3, 96, 96), 3, 8
    alg, orc, cfg = make_pair(obs_shape, A, "type_2", B)
    kw = cnn_kwargs(obs_shape, A, "type_2", B, buffer_max_size=40)
    buf = HipReplayBuffer(**kw)
    assert buf.engine is alg.engine
    rng = np.random.default_rng(0)
    rows = []
    for i in range(55):   # wraps the ring
        s = (rng.random(obs_shape, dtype=np.float32), {}, rng.uniform(-1, 1, A).astype(np.float32), float(rng.standard_normal()),
             rng.random(obs_shape, dtype=np.float32), bool(rng.random() < 0.3), np.float32(0.0), {})
        rows.append(s)
    buf.add_batch(rows[:25])
    buf.add_batch(rows[25:])
    assert (buf.size, buf.ptr) == (40, 15)
    ring = {}
    for i, s in enumerate(rows):
        ring[i % 40] = s
    np.random.seed(4)
    want_idx = np.random.randint(0, 40, size=B)
    np.random.seed(4)
    batch = buf.sample_batch(B)
    got = {k: batch[k].numpy() for k in ("obs", "obs2", "act", "rew", "done")}
    for r, i in enumerate(want_idx):
        s = ring[int(i)]
        assert np.array_equal(got["obs"][r], s[0]) and np.array_equal(got["obs2"][r], s[4])
        assert np.array_equal(got["act"][r], s[2]) and got["rew"][r] == np.float32(s[3]) and got["done"][r] == float(s[5])
    # sampler feed: conv stack + twin MLPs of the ONLINE policy through dsact_policy_forward
    obs = torch.as_tensor(rng.random((5,) + obs_shape, dtype=np.float32))
    with torch.no_grad():
        want = orc._pi(obs, orc.p["policy"])
    lg = alg.networks.policy(obs)
    assert lg.shape == want.shape
    assert float((lg.cpu() - want).abs().max()) < 2e-5


def test_cnn_load_batch_from_cuda_tensors_equals_host_staging():
    """dsact_load_batch with device pointers (the reference trainer's `.cuda()` image batch) stages the same
    pixel-major images and action columns as the host path."""
    from oracle.dsact_oracle_cnn import conv_out_hw, cnn_config, synth_image_batch
    from dsact.engine import DsactEngine

    cfg = cnn_config((3, 96, 96), 3, "type_2")
    B = 8
    data = synth_image_batch(cfg, B, seed=3)
    outs = []
    for on_gpu in (False, True):
        e = DsactEngine(cfg["obs_dim"], 3, list(cfg["hidden"]), B, conv_type="type_2")
        src = {k: (v.cuda() if on_gpu else v.numpy()) for k, v in data.items()}
        e.load_batch(src["obs"], src["act"], src["rew"], src["obs2"], src["done"])
        outs.append(e.read_batch(with_logp=False))
        e.close()
    for k in ("obs", "act", "rew", "obs2", "done"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
        assert np.array_equal(outs[0][k].reshape(-1), data[k].numpy().reshape(-1)), k


def _cnn_ring_alg(B, seed, rows=96):
    """DSAC_V2 with CNN nets, a filled image replay ring, an index table and the device RNG: ready for graph replays."""
    alg, _, cfg = make_pair((3, 96, 96), 3, "type_2", B, seed=seed)
    e = alg.engine
    e.set_device_rng(4242)
    e.buffer_create(rows)
    g = torch.Generator(device="cuda").manual_seed(9)
    O = 3 * 96 * 96
    e.buffer_fill_device(0, torch.rand(rows, O, device="cuda", generator=g), torch.rand(rows, 3, device="cuda", generator=g) * 2 - 1,
                         torch.randn(rows, device="cuda", generator=g), torch.rand(rows, O, device="cuda", generator=g),
                         (torch.rand(rows, device="cuda", generator=g) < .1).float())
    np.random.seed(2)
    e.upload_index_table(np.random.randint(0, rows, size=(6, B)))
    return alg


@pytest.mark.parametrize("B", [16, 64])
def test_cnn_twin_trunk_launch_forms_agree(B, monkeypatch):
    """The twin trunks as chain units in their three launch forms -- both trunks of a net in one workgroup (DSACT_TWIN_SEQ),
    the trunks as workgroups of their own with groups A and B as two launches (DSACT_TWIN_NO_MERGE), and everything in one
    forward launch (default) -- are the same arithmetic: parameters, targets and optimiser state bit for bit."""
    states = []
    for env in ({"DSACT_TWIN_SEQ": "1"}, {"DSACT_TWIN_NO_MERGE": "1"}, {}):
        for k in ("DSACT_TWIN_SEQ", "DSACT_TWIN_NO_MERGE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        alg = _cnn_ring_alg(B, seed=5)
        e = alg.engine
        assert e.chain_active
        ms = e.time_steps(0, 5, use_graph=False)
        assert ms > 0
        e.sync()
        states.append({n: getattr(e, n).clone() for n in ("online", "target", "adam_m", "adam_v")})
        assert torch.isfinite(states[-1]["online"]).all()
    for s in states[1:]:
        for n in s:
            assert torch.equal(states[0][n], s[n]), n


def test_cnn_graph_replay_equals_eager_steps():
    """hipGraph replays of the CNN update (image gather + conv stacks + twin-trunk chains + conv backward per update) == eager
    updates, bit for bit."""
    algs = []
    for mode in ("eager", "graph"):
        alg = _cnn_ring_alg(32, seed=6)
        e = alg.engine
        if mode == "graph":
            e.graph_build(3)
            e.graph_run(0, 6)
        else:
            assert e.time_steps(0, 6, use_graph=False) > 0
        e.sync()
        algs.append(alg)
    for name in ("online", "target", "adam_m", "adam_v"):
        assert torch.equal(getattr(algs[0].engine, name), getattr(algs[1].engine, name)), name
    assert algs[0].engine.get_state() == algs[1].engine.get_state()


def test_cnn_data_parallel_halves_equal_fused_steps():
    """The data-parallel seams on the CNN chain path (critic half -> all-reduce -> actor half -> all-reduce -> streaming Adam; world
    size 1) == the fused eager updates, bit for bit: the split flow forms dL/d features per half (dfeat_q, dfeat_pi) where the
    fused flow has one launch for the three nets."""
    import torch.distributed as dist
    from dsact.dp import DataParallelUpdater

    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29537")
        dist.init_process_group("gloo", rank=0, world_size=1)
        created = True
    try:
        a1 = _cnn_ring_alg(16, seed=7)
        assert a1.engine.time_steps(0, 4, use_graph=False) > 0
        a1.engine.sync()
        for overlap in (False, True):
            a2 = _cnn_ring_alg(16, seed=7)
            e = a2.engine
            dp = DataParallelUpdater(e, broadcast_tensors=(e.online, e.target, e.adam_m, e.adam_v), overlap=overlap)
            dp.force_collective = True
            e.dp_begin(0)
            for _ in range(4):
                dp.step()
            torch.cuda.synchronize()
            for name in ("online", "target", "adam_m", "adam_v"):
                assert torch.equal(getattr(a1.engine, name), getattr(e, name)), (name, overlap)
            assert a1.engine.get_state() == e.get_state()
    finally:
        if created:
            dist.destroy_process_group()


def test_cnn_twin_trunk_handover_timeout_fails_the_call_and_falls_back():
    """A first trunk that never raises its flag (debug switch): its partner gives up after the bounded spin, the next
    synchronising entry point FAILS the call, the handle refuses to train on until the state is restored, and falls back to
    the form without in-launch waits (both trunks of a net in one workgroup, groups A and B as two launches) -- from restored
    state bit-identical to an engine that never failed."""
    from dsact._ffi import DsactError

    alg, ref = _cnn_ring_alg(16, seed=8), _cnn_ring_alg(16, seed=8)
    e, r = alg.engine, ref.engine
    assert e.debug_get("twin_par") == 3.0
    snap = {k: v.clone() for k, v in alg.networks.state_dict().items()}
    arenas = {n: getattr(e, n).clone() for n in ("adam_m", "adam_v")}
    state = e.get_state()
    e.debug_set("withhold_flag", 1)
    with pytest.raises(DsactError, match="hand-over timed out"):
        e.time_steps(0, 1, use_graph=False)   # (raised here or by the next synchronising entry point)
        e.sync()
    assert e.debug_get("handoff_failures") == 1.0 and e.debug_get("twin_par") == 0.0 and e.debug_get("state_invalid") == 1.0
    with pytest.raises(DsactError, match="invalid after a hand-over timeout"):
        e.time_steps(0, 1, use_graph=False)
    r.time_steps(0, 1, use_graph=False)   # the same index-table cursor as the failed engine
    r.sync()
    for a_, x in ((alg, e), (ref, r)):
        a_.networks.load_state_dict(snap)
        for n, t in arenas.items():
            getattr(x, n).copy_(t)
        torch.cuda.synchronize()
        x.set_state(adam_steps=state["adam_steps"], mean_std=state["mean_std"])
    assert e.debug_get("state_invalid") == 0.0
    names = [k for k, _, _ in e.profile_step(0)]
    assert "chain_fwd_a" in names and "chain_fwd_b" in names
    r.profile_step(0)
    for x in (e, r):
        x.time_steps(0, 3, use_graph=False)
        x.sync()
    for name in ("online", "target", "adam_m", "adam_v"):
        assert torch.equal(getattr(e, name), getattr(r, name)), name
