"""dsact_act_sample_batch (csrc/dsact_act_batch.h) and the vectorised sampler on the GPU: the batched acting forward
against the torch module forward + the distribution's closed form, against the per-row call, row independence, live
weights behind unsynchronised updates, and HipVecOffSampler end to end."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs
from test_hip_parity import make_pair
from test_host_acting import close

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu


def _cpu_twin(alg, kw, module="dsac_v2_hip"):
    """an unattached CPU container holding the engine's current policy weights: the torch module forward"""
    alg.engine.sync()
    ref = __import__(module).ApproxContainer(**kw)
    ref.load_state_dict({k: v.detach().cpu() for k, v in alg.networks.state_dict().items()})
    return ref


def _reference(ref, obs, eps):
    """(action[n, A], logp[n], logits[n, 2A]) of policy(obs) and the distribution's sample with the draws eps"""
    with torch.no_grad():
        lg = ref.policy(torch.from_numpy(obs))
        dist = ref.create_action_distributions(lg)
        x = dist.mean + torch.from_numpy(eps) * dist.std
        if type(dist).__name__ == "GaussDistribution":
            a, lp = x, dist._base_log_prob(x)
        else:
            a, lp = dist._squash(x)
    return a.numpy(), lp.numpy(), lg.numpy()


def _check(a, lp, ra, rlp, rlg, lim, gauss, tag):
    for i in range(a.shape[0]):
        if gauss:
            np.testing.assert_allclose(a[i], ra[i], atol=1e-5, rtol=1e-5, err_msg=str((tag, i)))
            assert abs(float(lp[i]) - float(rlp[i])) <= 5e-4, (tag, i)
        else:
            close((a[i], float(lp[i]), rlg[i]), (ra[i], float(rlp[i]), rlg[i]), lim, (tag, i))


MATRIX = [
    (376, 17, (256, 256, 256), 256, 0.4, {}),
    (5, 1, (33,), 7, 2.0, {}),
    (24, 6, (128, 128), 64, 1.0, {"policy_std_type": "parameter"}),
    (24, 6, (64, 64), 64, 0.4, {"policy_act_distribution": "GaussDistribution"}),
    (16, 4, (64, 64), 64, 0.4, {"policy_hidden_sizes": [96, 40]}),
    (16, 4, (64, 64), 64, 0.4, {"policy_hidden_activation": "tanh"}),
    (24, 6, (64, 64), 64, 0.4, {"policy_output_activation": "tanh", "value_output_activation": "tanh"}),
    (24, 6, (64, 64), 64, 0.4, {"policy_output_activation": "sigmoid", "policy_std_type": "parameter"}),
    (24, 6, (64, 64), 64, 0.4, {"policy_output_activation": "gelu"}),
    (24, 6, (64, 64), 64, 0.4, {"policy_std_type": "mlp_separated"}),
    (24, 6, (96, 96), 64, 0.4, {"policy_std_type": "mlp_separated", "policy_hidden_activation": "relu"}),
    (17, 6, (64, 64), 64, 0.4, {}),
    (3, 2, (64, 64, 64, 64, 64), 64, 1.0, {}),        # 5 hidden layers: beyond the one-launch acting forward
    (900, 8, (64, 64), 64, 0.4, {}),                   # observation wider than the one-launch forward's 768 floats
    (20, 5, (64, 64), 64, 0.4, {"hip_pad_widths": True, "policy_hidden_sizes": [50, 70]}),   # zero-padded storage
]


@pytest.mark.parametrize("O,A,hid,B,lim,over", MATRIX)
def test_batch_equals_module_forward_and_reference_sample(O, A, hid, B, lim, over):
    alg, _ = make_pair(O, A, hid, B, act_limit=lim, seed=61, **over)
    e = alg.engine
    ref = _cpu_twin(alg, hip_kwargs(O, A, hid, B, act_limit=lim, **over))
    gauss = over.get("policy_act_distribution") == "GaussDistribution"
    rng = np.random.default_rng(3)
    for n in ((2, 7, 16, 64, 257, 1000, 1500) if O == 376 else (7, 64, 300)):
        obs = (3.0 * rng.standard_normal((n, O))).astype(np.float32)
        eps = rng.standard_normal((n, A)).astype(np.float32)
        a, lp = e.act_sample_batch(obs, eps)
        assert a.shape == (n, A) and lp.shape == (n,)
        _check(a, lp, *_reference(ref, obs, eps), lim, gauss, (n, O, A, hid))
        if n == 7:   # device-resident inputs: the same rows by device address
            a2, lp2 = e.act_sample_batch(torch.from_numpy(obs).cuda(), torch.from_numpy(eps).cuda())
            assert np.array_equal(a, a2) and np.array_equal(lp, lp2)
    assert e.debug_get("act_batch_calls") >= 3


def test_dsac_v1_handle():
    from test_hip_v1_parity import make_pair as make_v1

    O, A, hid, B = 24, 6, (64, 64), 64
    alg, _ = make_v1(O, A, hid, B, seed=5)
    ref = _cpu_twin(alg, hip_kwargs(O, A, hid, B, algorithm="DSAC_V1_HIP", TD_bound=10.0), module="dsac_v1_hip")
    rng = np.random.default_rng(4)
    obs = rng.standard_normal((33, O)).astype(np.float32)
    eps = rng.standard_normal((33, A)).astype(np.float32)
    a, lp = alg.engine.act_sample_batch(obs, eps)
    _check(a, lp, *_reference(ref, obs, eps), 0.4, False, "v1")


def test_batch_rows_equal_single_row_calls():
    alg, _ = make_pair(376, 17, (256, 256, 256), 256, seed=61)
    e = alg.engine
    ref = _cpu_twin(alg, hip_kwargs(376, 17, (256, 256, 256), 256))
    rng = np.random.default_rng(5)
    obs = rng.standard_normal((16, 376)).astype(np.float32)
    eps = rng.standard_normal((16, 17)).astype(np.float32)
    a, lp = e.act_sample_batch(obs, eps)
    lg = _reference(ref, obs, eps)[2]
    for i in range(16):
        a1, lp1 = e.act_sample(obs[i], eps[i])
        close((a[i], float(lp[i]), lg[i]), (a1.copy(), float(lp1[0]), lg[i]), 0.4, i)


def test_row_results_do_not_depend_on_the_batch():
    alg, _ = make_pair(376, 17, (256, 256, 256), 256, seed=7)
    e = alg.engine
    rng = np.random.default_rng(6)
    obs = rng.standard_normal((1100, 376)).astype(np.float32)
    eps = rng.standard_normal((1100, 17)).astype(np.float32)
    a_all, lp_all = e.act_sample_batch(obs, eps)          # 1100 rows: two chunks inside the call
    j = 123
    for n in (1, 2, 7, 31, 33, 64, 300, 1024, 1030):
        for pos in sorted({0, n // 2, n - 1}):
            idx = rng.integers(0, 1100, n)
            idx[pos] = j
            a, lp = e.act_sample_batch(obs[idx], eps[idx])
            assert np.array_equal(a[pos], a_all[j]) and lp[pos] == lp_all[j], (n, pos)
    assert np.array_equal(a_all[1024:], e.act_sample_batch(obs[1024:], eps[1024:])[0])


def test_batch_acts_with_the_weights_of_the_last_enqueued_update():
    O, A, hid, B, N = 16, 4, (64, 64), 64, 1024
    alg, _ = make_pair(O, A, hid, B, seed=4)
    e = alg.engine
    kw = hip_kwargs(O, A, hid, B)
    e.set_device_rng(11)
    e.buffer_create(N)
    g = torch.Generator(device="cuda").manual_seed(1)
    e.buffer_fill_device(0, torch.randn(N, O, device="cuda", generator=g), torch.rand(N, A, device="cuda", generator=g) - .5,
                         torch.randn(N, device="cuda", generator=g), torch.randn(N, O, device="cuda", generator=g),
                         (torch.rand(N, device="cuda", generator=g) < .05).float())
    np.random.seed(1)
    rows = np.random.randint(0, N, size=(8, B))
    e.upload_index_table(rows)
    rng = np.random.default_rng(8)
    obs = rng.standard_normal((40, O)).astype(np.float32)
    eps = rng.standard_normal((40, A)).astype(np.float32)
    prev = e.act_sample_batch(obs, eps)[0]

    def check(tag):
        nonlocal prev
        a, lp = e.act_sample_batch(obs, eps)       # right behind the enqueue: no synchronisation in between
        _check(a, lp, *_reference(_cpu_twin(alg, kw), obs, eps), 0.4, False, tag)
        assert not np.array_equal(a, prev), tag
        prev = a

    e.gather(rows[0]); e.step(0)
    check("eager step")
    e.run_group(5, rows[:5])
    check("group replay")
    e.graph_build(4)
    e.graph_run(10, 8)
    check("graph replay")


def test_local_update_then_vectorised_sample():
    """DSAC_V2_HIP.local_update left unsynchronised, then a HipVecOffSampler step on its networks"""
    from training.hip_vec_sampler import HipVecOffSampler
    from test_hip_groups import _ToyEnv

    alg, _ = make_pair(16, 4, (64, 64), 32, act_limit=0.3, seed=62)
    smp = HipVecOffSampler(envs=[_ToyEnv() for _ in range(8)], networks=alg.networks, sample_batch_size=8, action_type="continu",
                           hip_vec_act="gpu")
    torch.manual_seed(0)
    b0, _ = smp.sample()
    rng = np.random.default_rng(0)
    data = {"obs": rng.standard_normal((32, 16)).astype(np.float32), "act": (0.3 * rng.uniform(-1, 1, (32, 4))).astype(np.float32),
            "rew": rng.standard_normal(32).astype(np.float32), "obs2": rng.standard_normal((32, 16)).astype(np.float32),
            "done": np.zeros(32, np.float32)}
    alg.local_update({k: torch.from_numpy(v) for k, v in data.items()}, 0)
    smp.envs = [_ToyEnv() for _ in range(8)]
    smp.obs[...] = _ToyEnv().reset()[0]
    torch.manual_seed(0)
    b1, _ = smp.sample()
    obs = b1.packed[0]
    torch.manual_seed(0)
    eps = torch.randn(8, 4).numpy()
    ra, rlp, rlg = _reference(_cpu_twin(alg, hip_kwargs(16, 4, (64, 64), 32, act_limit=0.3)), obs, eps)
    _check(b1.packed[1], b1.packed[5], ra, rlp, rlg, 0.3, False, "local_update")
    assert not np.array_equal(b0.packed[1], b1.packed[1])


def test_vec_sampler_n1_is_hip_off_sampler_bitwise():
    from plugin import create_sampler
    from training.hip_sampler import HipOffSampler

    alg, _ = make_pair(376, 17, (256, 256, 256), 256, seed=9)
    kw = hip_kwargs(376, 17, (256, 256, 256), 256, env_id="synth_humanoid", sample_batch_size=20, seed=5)
    out = []
    for make in (lambda: HipOffSampler(**kw), lambda: create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=1, **kw)):
        torch.manual_seed(1)
        smp = make()
        smp.networks = alg.networks
        torch.manual_seed(2)
        out.append([smp.sample()[0] for _ in range(3)])
    for x, y in zip(*out):
        assert x.packed is not None and y.packed is not None
        for p, q in zip(x.packed, y.packed):
            assert np.array_equal(p, q)


def test_vec_sampler_n8_matches_per_environment_reconstruction():
    from plugin import create_sampler
    from synth_humanoid_data import SynthHumanoid

    hid = (256, 256, 256)
    alg, _ = make_pair(376, 17, hid, 256, seed=10)
    kw = hip_kwargs(376, 17, hid, 256, env_id="synth_humanoid", sample_batch_size=32, seed=20, hip_vec_gpu_min_envs=8)
    smp = create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=8, **kw)
    smp.networks = alg.networks
    assert smp.route() == "gpu"
    torch.manual_seed(3)
    batch, _ = smp.sample()
    ref = _cpu_twin(alg, kw)
    envs = [SynthHumanoid(seed=20 + i) for i in range(8)]
    obs = np.stack([e.reset()[0] for e in envs])
    torch.manual_seed(3)
    for t in range(4):
        eps = torch.randn(8, 17).numpy()
        ra, rlp, rlg = _reference(ref, obs, eps)
        rows = slice(8 * t, 8 * (t + 1))
        np.testing.assert_array_equal(batch.packed[0][rows], obs)
        _check(batch.packed[1][rows], batch.packed[5][rows], ra, rlp, rlg, 0.4, False, t)
        obs = np.stack([e.step(np.clip(a, -0.4, 0.4))[0] for e, a in zip(envs, batch.packed[1][rows])])
        np.testing.assert_array_equal(batch.packed[3][rows], obs)


def test_trainer_with_vec_sampler_ring_rows_are_the_sampled_transitions(tmp_path):
    import plugin

    kw = hip_kwargs(376, 17, (256, 256, 256), 256, env_id="synth_humanoid", sample_batch_size=32, reward_scale=0.5,
                    buffer_warm_size=256, buffer_max_size=10000, max_iteration=50, log_save_interval=1000,
                    apprfunc_save_interval=10000, eval_interval=10000, num_eval_episode=1, ini_network_dir=None,
                    save_folder=str(tmp_path), seed=3, sample_interval=1, sampler_name="hip_vec_off_sampler", vector_env_num=8)
    torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
    alg = plugin.create_alg(**kw)
    sampler = plugin.create_sampler(**kw)
    buf = plugin.create_buffer(**kw)
    seen = []
    orig = sampler.sample

    def rec():
        b, tb = orig()
        seen.append([a.copy() for a in b.packed])
        return b, tb

    sampler.sample = rec
    tr = plugin.create_trainer(alg, sampler, buf, plugin.create_evaluator(**kw), **kw)
    tr.train()
    e = alg.engine
    n = sum(len(s[0]) for s in seen)
    assert n == 256 + 50 * 32 and e.buffer_size == n
    want = [np.concatenate([s[k] for s in seen]) for k in range(6)]
    for r0 in range(0, n - 255, 256):
        e.gather(np.arange(r0, r0 + 256))
        got = e.read_batch(with_logp=True)
        for k, key in enumerate(("obs", "act", "rew", "obs2", "done", "logp")):
            np.testing.assert_array_equal(np.asarray(got[key]).reshape(256, -1), want[k][r0:r0 + 256].reshape(256, -1), err_msg=key)
    assert np.isfinite(list(e.read_stats().values())).all()


def test_cnn_policy_acts_through_the_module_forward():
    import plugin
    from dsact._ffi import DsactError
    from test_hip_cnn_parity import cnn_kwargs

    kw = cnn_kwargs((3, 96, 96), 3, "type_2", 8, env_id="synth_blob", sample_batch_size=8, seed=4, strict_rng=False)
    torch.manual_seed(0)
    alg = plugin.create_alg(**kw)
    with pytest.raises(DsactError):
        alg.engine.act_sample_batch(np.zeros((2, 3 * 96 * 96), np.float32), np.zeros((2, 3), np.float32))
    smp = plugin.create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=4, **kw)
    smp.networks = alg.networks
    assert smp.route() == "module"
    torch.manual_seed(6)
    batch, _ = smp.sample()
    assert len(batch) == 8 and batch.packed[0].shape == (8, 3 * 96 * 96)
    torch.manual_seed(6)
    with torch.no_grad():
        lg = alg.networks.policy(torch.from_numpy(batch.packed[0][:4].reshape(4, 3, 96, 96)))
        dist = alg.networks.create_action_distributions(lg)
        a, lp = dist.sample()
    np.testing.assert_array_equal(batch.packed[1][:4], a.numpy())
    np.testing.assert_array_equal(batch.packed[5][:4], lp.numpy())
