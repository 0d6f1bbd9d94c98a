"""Exploration noise on the GPU (dsact_set_explore_noise, k_act_batch_out<false, true, true>; the
reference's GaussNoise, training/off_sampler.py:58-65 and utils/explore_noise.py:17-23):

  1. off is today's result, bit for bit, before and after a noise-on call; the debug counter;
  2. the drawn normals equal the float64 restatement on stream 6 (tests/test_explore_noise_host.py pins its words) within the
     NOISE_GATE of tests/test_tensor_sampler_gpu.py -- the same fp32 Box-Muller code on another stream id;
  3. general parameters: logp untouched, clipped = clip(action), a std == 0 column exact, the others within a derived bound;
  4. the exploration stream is not eps's stream; step and seed reach it;  5. a row does not depend on the batch or the chunk;
  6. a CNN handle, from fp32 and from byte frames;  7. refusals leave the handle usable;
  8. HipTensorEnvSampler: the ring gets the un-clipped noised action, the environment its clip;
  9. the host routes on a real engine add NumPy's draw;  10. the serial and the overlapped trainer run and repeat bitwise.
Every test fails on a tree without the feature (NotImplementedError, or no such symbol).
"""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs
from test_hip_parity import make_pair
from test_tensor_sampler_gpu import NOISE_GATE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

SEED = 0x5DEECE66D1234567
F32 = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _act_device(e, obs, eps, step=0):
    """act_sample_device on host arrays (float32 rows / frames, or uint8 frames): (action, clipped, logp) as numpy"""
    n = obs.shape[0]
    o = _dev(obs)
    ep = _dev(eps) if eps is not None else None
    act = torch.empty(n, e.act_dim, device="cuda")
    clip, lp = torch.empty_like(act), torch.empty(n, device="cuda")
    torch.cuda.synchronize()                       # the inputs were produced on torch's stream; the call runs on the engine's
    e.act_sample_device(o, ep, step, act, clip, lp)
    e.sync()
    return act.cpu().numpy(), clip.cpu().numpy(), lp.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _bound(std, clean, mean, sz):
    """|action - (clean + mean + std * z_ref)| <=: the drawn normal's gate times std, plus the two fp32 roundings of
    fma(std, z, mean) and of the sum with the clean action (each <= 2^-24 relative to its result) with margin"""
    return std * NOISE_GATE + 4 * F32 * (np.abs(clean) + np.abs(mean) + np.abs(sz))


def _zero_output_gauss(O, A, seed=2):
    """a GaussDistribution policy whose output layer is zero: mean 0, std exp(0) = 1 -- the sample IS eps, exactly"""
    alg, _ = make_pair(O, A, (64, 64), 64, seed=seed, policy_act_distribution="GaussDistribution")
    params = dict(alg.networks.policy.named_parameters())
    last = max(int(k.split(".")[1]) for k in params if k.startswith("policy."))
    with torch.no_grad():
        params["policy.%d.weight" % last].zero_()
        params["policy.%d.bias" % last].zero_()
    torch.cuda.synchronize()
    return alg.engine


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def test_off_is_todays_result_and_the_counter_reports_the_mode():
    O, A, n = 17, 6, 33
    alg, _ = make_pair(O, A, (64, 64), 64, seed=61)
    e = alg.engine
    rng = np.random.default_rng(3)
    obs = (3.0 * rng.standard_normal((n, O))).astype(np.float32)
    eps = rng.standard_normal((n, A)).astype(np.float32)
    ra, rlp = e.act_sample_batch(obs, eps)
    e.set_act_rng(SEED)
    assert e.debug_get("explore_noise") == 0.0                      # every handle starts with the noise off
    e.set_explore_noise(None)
    assert e.debug_get("explore_noise") == 0.0
    a, c, lp = _act_device(e, obs, eps)
    assert np.array_equal(_bits(a), _bits(ra)) and np.array_equal(_bits(lp), _bits(rlp))
    e.set_explore_noise(0.0, 0.5)
    assert e.debug_get("explore_noise") == 1.0
    a1, c1, lp1 = _act_device(e, obs, eps)
    assert not np.array_equal(a1, ra) and np.array_equal(_bits(lp1), _bits(rlp))
    e.set_explore_noise(np.zeros(A), np.full(A, 0.5))
    assert e.debug_get("explore_noise") == float(A)
    a6 = _act_device(e, obs, eps)[0]
    assert not np.array_equal(a6, ra) and not np.array_equal(a6, a1)
    ha, hlp = e.act_sample_batch(obs, eps)                          # the host-returning call never adds noise
    assert np.array_equal(_bits(ha), _bits(ra)) and np.array_equal(_bits(hlp), _bits(rlp))
    e.set_explore_noise(None)
    assert e.debug_get("explore_noise") == 0.0
    a, c, lp = _act_device(e, obs, eps)
    assert np.array_equal(_bits(a), _bits(ra)) and np.array_equal(_bits(lp), _bits(rlp))
    assert np.array_equal(_bits(c), _bits(np.clip(a, e.act_low, e.act_high)))
    assert e.debug_get("act_dev_syncs") == 0.0


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [16, 6])
def test_the_draw_equals_the_float64_restatement(A):
    from training.hip_tensor_sampler import explore_noise_reference

    O, n = 16, 1030                                                 # 1030 rows: both sides of the 1024-row chunk
    e = _zero_output_gauss(O, A)
    e.set_act_rng(SEED)
    obs = np.random.default_rng(0).standard_normal((n, O)).astype(np.float32)
    zero = np.zeros((n, A), np.float32)                             # injected eps = 0: the clean action is exactly 0
    worst = 0.0
    for shared in (False, True):
        if shared:
            e.set_explore_noise(0.0, 1.0)
        else:
            e.set_explore_noise(np.zeros(A), np.ones(A))
        assert e.debug_get("explore_noise") == (1.0 if shared else float(A))
        for step in (2 ** 32 - 1, 2 ** 32, 0):
            a, c, lp = _act_device(e, obs, zero, step)
            want = explore_noise_reference(SEED, step, n, A, shared)
            diff = float(np.abs(a.astype(np.float64) - want).max())
            worst = max(worst, diff)
            assert np.isfinite(a).all() and diff <= NOISE_GATE, (shared, step, diff, NOISE_GATE)
            assert np.array_equal(_bits(c), _bits(np.clip(a, e.act_low, e.act_high)))
            if shared:
                assert (_bits(a) == _bits(a)[:, :1]).all(), step    # one normal per row in every column
            else:
                assert not (a == a[:, :1]).all()
    print("A = %d: max |kernel exploration normal - float64 restatement| = %.3e (gate %.3e)" % (A, worst, NOISE_GATE))
    assert e.debug_get("act_dev_syncs") == 0.0


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_general_parameters_against_a_clean_call():
    from training.hip_tensor_sampler import explore_noise_reference

    O, A, n, step = 17, 6, 33, 5
    alg, _ = make_pair(O, A, (64, 64), 64, act_limit=0.4, seed=61)
    e = alg.engine
    rng = np.random.default_rng(3)
    obs = (3.0 * rng.standard_normal((n, O))).astype(np.float32)
    eps = rng.standard_normal((n, A)).astype(np.float32)
    mean = np.array([0.05, -0.1, 0.0, 0.3, -0.02, 0.01], np.float32)
    std = np.array([0.3, 0.2, 0.5, 0.0, 1.0, 0.05], np.float32)     # one std == 0 column
    e.set_act_rng(SEED)
    clean, _, clean_lp = _act_device(e, obs, eps, step)
    e.set_explore_noise(mean, std)
    a, c, lp = _act_device(e, obs, eps, step)
    assert np.array_equal(_bits(lp), _bits(clean_lp))               # logp: the un-noised sample's
    assert np.array_equal(_bits(c), _bits(np.clip(a, e.act_low, e.act_high)))
    assert (a > e.act_high).any() and (a < e.act_low).any()         # (the +-0.4 limits are tight enough: rows clip)
    assert np.array_equal(_bits(a[:, 3]), _bits(clean[:, 3] + mean[3]))   # std == 0: fl32(clean + mean), no draw's trace
    sz = std.astype(np.float64) * explore_noise_reference(SEED, step, n, A, False)
    want = clean.astype(np.float64) + mean.astype(np.float64) + sz
    err = np.abs(a.astype(np.float64) - want)
    tol = _bound(std.astype(np.float64)[None, :], clean.astype(np.float64), mean.astype(np.float64)[None, :], sz)
    print("max |action - (clean + mean + std z_ref)| / bound = %.3f" % float((err / tol).max()))
    assert (err <= tol).all(), float((err / tol).max())
    assert e.debug_get("act_dev_syncs") == 0.0


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def test_the_exploration_stream_is_not_the_acting_stream():
    from training.hip_tensor_sampler import act_noise_reference, explore_noise_reference

    O, A, n, step = 16, 6, 64, 11
    e = _zero_output_gauss(O, A)
    e.set_act_rng(SEED)
    e.set_explore_noise(np.zeros(A), np.ones(A))
    obs = np.random.default_rng(0).standard_normal((n, O)).astype(np.float32)

    def noise(seed, st):
        e.set_act_rng(seed)
        a = _act_device(e, obs, None, st)[0]                        # eps drawn in the kernel too: action = eps + z
        return a.astype(np.float64) - act_noise_reference(seed, st, n, A)

    z = noise(SEED, step)
    assert float(np.abs(z - explore_noise_reference(SEED, step, n, A, False)).max()) <= 2 * NOISE_GATE
    assert float(np.abs(z).max()) > 1.0                             # (it is there, and it is not eps again)
    assert float(np.abs(z - act_noise_reference(SEED, step, n, A)).max()) > 1.0
    z_step, z_seed = noise(SEED, step + 1), noise(SEED ^ 1, step)
    assert float(np.abs(z_step - z).max()) > 1.0 and float(np.abs(z_seed - z).max()) > 1.0
    assert float(np.abs(z_step - explore_noise_reference(SEED, step + 1, n, A, False)).max()) <= 2 * NOISE_GATE
    assert float(np.abs(z_seed - explore_noise_reference(SEED ^ 1, step, n, A, False)).max()) <= 2 * NOISE_GATE


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
def test_a_row_does_not_depend_on_the_batch_or_the_chunk(shared):
    O, A = 17, 6
    alg, _ = make_pair(O, A, (64, 64), 64, seed=7)
    e = alg.engine
    e.set_act_rng(0x1234567887654321)
    if shared:
        e.set_explore_noise(0.1, 0.3)
    else:
        e.set_explore_noise(np.linspace(-0.1, 0.1, A), np.linspace(0.1, 0.6, A))
    obs = np.random.default_rng(6).standard_normal((1030, O)).astype(np.float32)
    for step in (0, 2 ** 32 + 5):
        big = _act_device(e, obs, None, step)
        small = _act_device(e, obs[:4], None, step)
        tail = _act_device(e, obs[1024:], None, step)               # rows 1024 .. 1029 as rows 0 .. 5 of another call: other noise
        for x, y, t in zip(big, small, tail):
            assert np.array_equal(_bits(x[:4]), _bits(y)), step
        assert not np.array_equal(big[0][1024:], tail[0])


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_cnn_handle_from_fp32_and_byte_frames():
    from test_tensor_image_gpu import BOOK, _make
    from training.hip_tensor_sampler import explore_noise_reference

    shape, A, n, step = (4, 84, 84), 2, 5, 3
    alg, _ = _make(shape, A, "type_1", book=BOOK)                    # a coded ring: byte frames are allowed
    e = alg.engine
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 256, (n,) + shape, dtype=np.uint8)
    frames = BOOK[codes]
    eps = rng.standard_normal((n, A)).astype(np.float32)
    mean, std = np.array([0.1, -0.2], np.float32), np.array([0.5, 0.25], np.float32)
    e.set_act_rng(SEED)
    clean, _, clean_lp = _act_device(e, frames, eps, step)
    e.set_explore_noise(mean, std)
    a, c, lp = _act_device(e, frames, eps, step)
    a8, c8, lp8 = _act_device(e, codes, eps, step)
    for x, y in ((a, a8), (c, c8), (lp, lp8)):
        assert np.array_equal(_bits(x), _bits(y))                   # byte frames: bit for bit the decoded frames' result
    assert np.array_equal(_bits(lp), _bits(clean_lp)) and np.array_equal(_bits(c), _bits(np.clip(a, e.act_low, e.act_high)))
    sz = std.astype(np.float64) * explore_noise_reference(SEED, step, n, A, False)
    err = np.abs(a.astype(np.float64) - (clean.astype(np.float64) + mean + sz))
    tol = _bound(std.astype(np.float64)[None, :], clean.astype(np.float64), mean.astype(np.float64)[None, :], sz)
    assert (err <= tol).all() and float(np.abs(a - clean).max()) > 0.1, float((err / tol).max())
    e.set_explore_noise(None)
    assert np.array_equal(_bits(_act_device(e, codes, eps, step)[0]), _bits(clean))
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from dsact._ffi import DsactError

    O, A, n = 17, 6, 8
    alg, _ = make_pair(O, A, (64, 64), 64, seed=4)
    e = alg.engine
    f = lambda *s: torch.zeros(*s, device="cuda")
    obs, eps, act, clip, lp = f(n, O), f(n, A), f(n, A), f(n, A), f(n)
    torch.cuda.synchronize()
    e.set_explore_noise(0.0, 0.1)
    with pytest.raises(DsactError, match="E_STATE.*dsact_set_act_rng"):
        e.act_sample_device(obs, eps, 0, act, clip, lp)            # no acting seed -- also with eps passed in
    e.set_act_rng(9)
    e.act_sample_device(obs, eps, 0, act, clip, lp)
    with pytest.raises(DsactError, match="E_INVALID"):
        e.set_explore_noise([0.0, 0.0], [1.0, 1.0])                # n = 2 on an A = 6 handle
    assert e.debug_get("explore_noise") == 1.0
    e.act_sample_device(obs, eps, 1, act, clip, lp)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(DsactError, match="E_INVALID"):
            e.set_explore_noise(0.0, bad)
        with pytest.raises(DsactError, match="E_INVALID"):
            e.set_explore_noise(np.zeros(A), np.r_[np.ones(A - 1), bad])
    with pytest.raises(DsactError, match="E_INVALID"):
        e.set_explore_noise(float("nan"), 1.0)
    with pytest.raises(ValueError):
        e.set_explore_noise(0.0, None)
    assert e.debug_get("explore_noise") == 1.0                      # a refused call changes nothing
    e.act_sample_device(obs, None, 2, act, clip, lp)
    e.sync()
    assert torch.isfinite(act).all() and torch.equal(clip, act.clamp(-0.4, 0.4)) and float(act.abs().max()) > 0.0
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
def _tensor_run(noise, record=None):
    import plugin
    from synth_tensor_humanoid import SynthTensorHumanoid

    O, A, N, S, B = 376, 17, 8, 32, 64
    kw = hip_kwargs(O, A, (64, 64), B, buffer_max_size=200, seed=5, sample_batch_size=S, strict_rng=False, noise_params=noise)
    torch.manual_seed(1)
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    env = SynthTensorHumanoid(N, device="cuda", seed=4, episode_limit=3)
    if record is not None:
        step = env.step
        env.step = lambda a: (record.append(a.clone()), step(a))[1]
    smp = plugin.create_sampler(sampler_name="hip_tensor_env_sampler", env=env, networks=alg.networks, **kw)
    batch, _ = smp.sample()
    e = alg.engine
    e.sync()
    host = [t.cpu().numpy().copy() for t in batch.device_columns]
    buf.add_batch(batch)
    e.gather(np.arange(B) % S)
    ring_act = np.asarray(e.read_batch(with_logp=True)["act"]).reshape(B, A)[:S].copy()
    assert e.debug_get("handoff_failures") == 0.0 and e.debug_get("act_dev_syncs") == 0.0
    assert e.debug_get("explore_noise") == (0.0 if noise is None else 1.0)
    return smp, host, ring_act


def test_tensor_sampler_stores_the_noised_action_and_steps_with_its_clip():
    from training.hip_tensor_sampler import explore_noise_reference

    N, A = 8, 17
    params = {"mean": 0.0, "std": 0.2}
    seen = []
    smp, host, ring_act = _tensor_run(params, seen)
    _, host2, ring2 = _tensor_run(dict(params))
    for x, y in zip(host, host2):
        assert np.array_equal(x, y)                                 # two fresh runs: bitwise equal
    assert np.array_equal(_bits(ring_act), _bits(ring2))
    act = host[1]
    assert len(seen) == 4
    for t, a in enumerate(seen):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(np.clip(act[t * N:(t + 1) * N], np.float32(-0.4), np.float32(0.4))))
    assert np.array_equal(_bits(ring_act), _bits(act)) and float(np.abs(act).max()) > 0.4       # the ring: un-clipped, noised
    smp0, clean, _ = _tensor_run(None)
    assert smp0.act_seed == smp.act_seed and np.array_equal(clean[0][:N], host[0][:N])          # the first step: same observations
    assert np.array_equal(_bits(clean[6][:N]), _bits(host[6][:N]))                              # logp: the un-noised sample's
    sz = 0.2 * explore_noise_reference(smp.act_seed, 0, N, A, True)
    c0 = clean[1][:N].astype(np.float64)
    err = np.abs(act[:N].astype(np.float64) - (c0 + sz))
    tol = _bound(0.2, c0, 0.0, sz)
    assert (err <= tol).all() and float(np.abs(c0).max()) <= 0.4, float((err / tol).max())


# ---- 9 -------------------------------------------------------------------------------------------------------------------------
HOST_PARAMS = [pytest.param({"mean": 0.05, "std": 0.3}, id="scalar"), pytest.param({"mean": [0.05], "std": [0.3]}, id="array")]


@pytest.mark.parametrize("params", HOST_PARAMS)
def test_fast_path_adds_numpys_draw(params):
    from training.hip_sampler import HipOffSampler

    alg, _ = make_pair(3, 1, (32, 32), 16, act_limit=2.0, seed=9)
    out = []
    for p in (params, None):
        kw = hip_kwargs(3, 1, (32, 32), 16, act_limit=2.0, env_id="synth_pendulum", sample_batch_size=1, seed=5, noise_params=p)
        torch.manual_seed(1)
        smp = HipOffSampler(**kw)
        smp.networks = alg.networks
        assert smp.per_row_engine() is alg.engine                   # the fast path
        torch.manual_seed(2)
        np.random.seed(3)
        out.append(smp.sample()[0])
    noised, twin = out
    np.random.seed(3)
    want = twin[0][2] + np.random.normal(params["mean"], params["std"])      # NumPy's own arithmetic and dtype
    assert noised[0][2].dtype == want.dtype and np.array_equal(noised[0][2], want)
    assert np.array_equal(noised.packed[1][0], want.astype(np.float32)) and np.array_equal(noised[0][6], twin[0][6])
    assert not np.array_equal(want.astype(np.float64), twin[0][2].astype(np.float64))


@pytest.mark.parametrize("route", ["gpu", "host"])
@pytest.mark.parametrize("params", HOST_PARAMS)
def test_vec_routes_add_the_rows_of_one_draw(params, route):
    from plugin import create_sampler

    N = 4
    alg, _ = make_pair(3, 1, (32, 32), 16, act_limit=2.0, seed=9)
    out = []
    for p in (params, None):
        kw = hip_kwargs(3, 1, (32, 32), 16, act_limit=2.0, env_id="synth_pendulum", sample_batch_size=N, seed=5, noise_params=p,
                        hip_vec_act=route)
        torch.manual_seed(1)
        smp = create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=N, **kw)
        smp.networks = alg.networks
        assert smp.route() == route
        torch.manual_seed(2)
        np.random.seed(3)
        out.append(smp.sample()[0])
    noised, twin = out
    np.random.seed(3)
    for i in range(N):
        want = twin[i][2] + np.random.normal(params["mean"], params["std"])  # row i: the i-th sequential draw
        assert noised[i][2].dtype == want.dtype and np.array_equal(noised[i][2], want), i
        assert np.array_equal(noised.packed[1][i], want.astype(np.float32)) and np.array_equal(noised[i][6], twin[i][6])


# ---- 10 ------------------------------------------------------------------------------------------------------------------------
def test_serial_trainer_runs_with_the_noised_tensor_sampler(tmp_path):
    import plugin
    from synth_tensor_humanoid import SynthTensorHumanoid
    from training.hip_trainer import HipOffSerialTrainer, read_scalars

    O, A, N, S, K, iters, cap, warm = 376, 17, 16, 32, 8, 32, 1000, 64
    finals = []
    for run in range(2):
        folder = str(tmp_path / ("run%d" % run))
        kw = hip_kwargs(O, A, (64, 64), 64, buffer_max_size=cap, buffer_warm_size=warm, seed=3, sample_batch_size=S,
                        sample_interval=K, max_iteration=iters, log_save_interval=8, apprfunc_save_interval=100000,
                        eval_interval=100000, save_folder=folder, ini_network_dir=None, strict_rng=False, hip_device_indices=True,
                        reward_scale=0.25, sampler_name="hip_tensor_env_sampler", noise_params={"mean": 0.0, "std": 0.1})
        torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
        alg = plugin.create_alg(**kw)
        buf = plugin.create_buffer(**kw)
        smp = plugin.create_sampler(env=SynthTensorHumanoid(N, device="cuda", seed=4, episode_limit=50), **kw)
        tr = plugin.create_trainer(alg, smp, buf, None, **kw)
        assert type(tr) is HipOffSerialTrainer
        tr.train()
        e = alg.engine
        e.sync()
        assert e.debug_get("explore_noise") == 1.0 and e.debug_get("handoff_failures") == 0.0 and e.debug_get("act_dev_syncs") == 0.0
        scal = read_scalars(folder)
        assert len(scal["Loss/Critic loss-RL iter"]["y"]) >= 1
        for tag, d in scal.items():
            assert np.isfinite(d["y"]).all(), tag
        assert torch.isfinite(e.online).all()
        finals.append((e.online.cpu().clone(), e.target.cpu().clone(), e.adam_m.cpu().clone(), tuple(e.buffer_digest())))
    for x, y in zip(*finals):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y


def test_overlapped_trainer_runs_with_the_noised_host_sampler(tmp_path):
    import plugin
    from training.hip_async_trainer import HipOffAsyncTrainer

    O, A, S, K, iters = 376, 17, 16, 2, 16
    finals = []
    for run in range(2):
        kw = hip_kwargs(O, A, (64, 64), 64, env_id="synth_humanoid", buffer_max_size=1000, buffer_warm_size=64, seed=3,
                        sample_batch_size=S, sample_interval=K, max_iteration=iters, log_save_interval=8, apprfunc_save_interval=100000,
                        eval_interval=100000, save_folder=str(tmp_path / ("run%d" % run)), ini_network_dir=None, strict_rng=True,
                        trainer="hip_off_async_trainer", noise_params={"mean": 0.0, "std": 0.1})
        torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
        alg = plugin.create_alg(**kw)
        buf = plugin.create_buffer(**kw)
        smp = plugin.create_sampler(**kw)
        tr = plugin.create_trainer(alg, smp, buf, None, **kw)
        assert type(tr) is HipOffAsyncTrainer and smp.noise is not None and smp.per_row_engine() is alg.engine
        tr.train()
        e = alg.engine
        e.sync()
        assert e.debug_get("beh_holds") == iters // K and e.debug_get("handoff_failures") == 0.0 and torch.isfinite(e.online).all()
        assert e.debug_get("explore_noise") == 0.0                  # the host routes add their noise in Python
        finals.append((e.online.cpu().clone(), e.target.cpu().clone(), tuple(e.buffer_digest()), np.random.normal()))
    for x, y in zip(*finals):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y
