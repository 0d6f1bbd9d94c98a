"""Device-resident sampling on the GPU (csrc/dsact_act_batch.h kDev form, k_ring_commit, dsact_act_sample_device /
dsact_buffer_add_device, training/hip_tensor_sampler.py):

  4. with an injected device eps, action and logp equal dsact_act_sample_batch's bit for bit; clipped == np.clip(action);
  5. drawn noise: a row's result does not depend on N or on the chunk it falls in; the normals equal the float64 restatement of
     tests/test_tensor_sampler_host.py within the measured fp32 distance (see NOISE_GATE);
  6. the ring after wrapping adds == a NumPy restatement of the reference's store(), ptr / size after every add;
  7. a sample() makes no host round trip;
  8. HipOffSerialTrainer runs with the sampler; two runs from the same seeds end bitwise equal;
  9. refusals on the real engine leave the handle usable.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs
from test_hip_parity import make_pair

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "envs"))

pytestmark = pytest.mark.gpu

# max |kernel normal - float64 restatement| over the 1 015 808 draws of the test below, measured on an MI355X (DESIGN.md section
# 15). The kernel evaluates the map in fp32. The largest term is not the last bits of log / sin / cos but the uniform itself:
# (float)(w >> 8) + 0.5f is not representable once w >> 8 >= 2^23 and rounds to even, so u moves by 2^-25 -- for the last value,
# u0 = 1 - 2^-25 becomes 1.0 and r = sqrt(-2 ln u0) = 2.44e-4 becomes 0. The gate is 4x the measurement.
MEASURED_NOISE_DIFF = 2.362e-4
NOISE_GATE = 4.0 * MEASURED_NOISE_DIFF


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _act_device(e, obs, eps, step=0):
    """act_sample_device on host arrays: (action, clipped, logp) as numpy"""
    n = obs.shape[0]
    o = _dev(obs)
    ep = _dev(eps) if eps is not None else None
    act = torch.empty(n, e.act_dim, device="cuda")
    clip, lp = torch.empty_like(act), torch.empty(n, device="cuda")
    torch.cuda.synchronize()                       # the inputs were produced on torch's stream; the call runs on the engine's
    e.act_sample_device(o, ep, step, act, clip, lp)
    e.sync()
    return act.cpu().numpy(), clip.cpu().numpy(), lp.cpu().numpy()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O,A,hid,B,over", [
    (376, 17, (256, 256, 256), 256, {}),                                                           # the BASELINE policy
    (17, 6, (64, 64), 64, {}),
    (24, 6, (64, 64), 64, {"policy_std_type": "mlp_separated"}),
    (24, 6, (64, 64), 64, {"policy_output_activation": "tanh", "value_output_activation": "tanh"}),
    (24, 6, (64, 64), 64, {"policy_act_distribution": "GaussDistribution"}),
])
def test_injected_eps_is_bitwise_the_batch_call(O, A, hid, B, over):
    alg, _ = make_pair(O, A, hid, B, seed=61, **over)
    e = alg.engine
    rng = np.random.default_rng(3)
    lo, hi = e.act_low, e.act_high
    for n in (1, 33, 256, 1500):
        obs = (3.0 * rng.standard_normal((n, O))).astype(np.float32)
        eps = rng.standard_normal((n, A)).astype(np.float32)
        calls = e.debug_get("act_dev_calls")
        a, c, lp = _act_device(e, obs, eps)
        assert e.debug_get("act_dev_calls") - calls == (n + 1023) // 1024
        ra, rlp = e.act_sample_batch(obs, eps)
        assert np.array_equal(a.view(np.uint32), ra.view(np.uint32)), (n, np.abs(a - ra).max())
        assert np.array_equal(lp.view(np.uint32), rlp.view(np.uint32)), (n, np.abs(lp - rlp).max())
        assert np.array_equal(c.view(np.uint32), np.clip(a, lo, hi).view(np.uint32)), n
        if over.get("policy_act_distribution") == "GaussDistribution":
            assert (a > hi).any() and (a < lo).any()           # the clip had something to do
    assert e.debug_get("act_dev_syncs") == 0.0


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_drawn_noise_does_not_depend_on_the_batch_around_a_row():
    O, A = 376, 17
    alg, _ = make_pair(O, A, (256, 256, 256), 256, seed=7)
    e = alg.engine
    e.set_act_rng(0x1234567887654321)
    rng = np.random.default_rng(6)
    obs = rng.standard_normal((1500, O)).astype(np.float32)
    for step in (0, 3, 2 ** 32 + 5):
        big = _act_device(e, obs, None, step)                     # 1500 rows: two chunks inside the call
        for n in (4, 1024, 1030):
            small = _act_device(e, obs[:n], None, step)
            for x, y in zip(big, small):
                assert np.array_equal(x[:n], y), (step, n)
    a0, a1 = _act_device(e, obs, None, 0)[0], _act_device(e, obs, None, 1)[0]
    assert not np.array_equal(a0, a1)                             # the step reaches the counter ...
    e.set_act_rng(0x1234567887654320)
    assert not np.array_equal(a0, _act_device(e, obs, None, 0)[0])   # ... and the seed the key


def test_drawn_normals_equal_the_float64_restatement():
    """A GaussDistribution policy whose output layer is zero has mean 0 and std exp(0) = 1: its action IS the drawn eps
    (0 + eps * 1, exact in fp32). 31 acting steps of 2048 rows x 16 dimensions = 1 015 808 draws, rows on both sides of the chunk
    cap. Measured on an MI355X: max |kernel - float64| = MEASURED_NOISE_DIFF; the gate is 4x that (fp32 log / sin / cos have
    implementation-dependent last bits)."""
    from training.hip_tensor_sampler import act_noise_reference

    O, A, n, steps, seed = 16, 16, 2048, 31, 0x5DEECE66D1234567
    alg, _ = make_pair(O, A, (64, 64), 64, seed=2, policy_act_distribution="GaussDistribution")
    e = alg.engine
    params = dict(alg.networks.policy.named_parameters())
    last = max(int(k.split(".")[1]) for k in params if k.startswith("policy."))
    with torch.no_grad():
        params["policy.%d.weight" % last].zero_()
        params["policy.%d.bias" % last].zero_()
    torch.cuda.synchronize()
    e.set_act_rng(seed)
    obs = _dev(np.random.default_rng(0).standard_normal((n, O)).astype(np.float32))
    act = torch.empty(steps, n, A, device="cuda")
    clip, lp = torch.empty(n, A, device="cuda"), torch.empty(n, device="cuda")
    torch.cuda.synchronize()
    first = 2 ** 32 - 10                                          # the step counter crosses 2^32 on the way
    for t in range(steps):
        e.act_sample_device(obs, None, first + t, act[t], clip, lp)
    e.sync()
    got = act.cpu().numpy().astype(np.float64)
    want = np.stack([act_noise_reference(seed, first + t, n, A) for t in range(steps)])
    diff = float(np.abs(got - want).max())
    print("max |kernel normal - float64 restatement| over %d draws: %.3e (gate %.3e); max |z| %.3f, mean %.2e, var %.5f"
          % (got.size, diff, NOISE_GATE, np.abs(want).max(), got.mean(), got.var()))
    assert got.size >= 10 ** 6 and np.isfinite(got).all()
    assert diff <= NOISE_GATE, (diff, NOISE_GATE)


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
class _HostRing:
    """training/replay_buffer.py:58-79 restated: store() row by row with ptr = (ptr + 1) % N, size = min(size + 1, N)"""

    def __init__(self, cap, O, A):
        self.buf = {"obs": np.zeros((cap, O), np.float32), "obs2": np.zeros((cap, O), np.float32), "act": np.zeros((cap, A), np.float32),
                    "rew": np.zeros(cap, np.float32), "done": np.zeros(cap, np.float32), "logp": np.zeros(cap, np.float32)}
        self.ptr, self.size, self.cap = 0, 0, cap

    def store(self, obs, act, rew, obs2, done, logp):
        for k, v in (("obs", obs), ("obs2", obs2), ("act", act), ("rew", rew), ("done", done), ("logp", logp)):
            self.buf[k][self.ptr] = v
        self.ptr = (self.ptr + 1) % self.cap
        self.size = min(self.size + 1, self.cap)


@pytest.mark.parametrize("O,A,hid", [(376, 17, (256, 256, 256)), (17, 6, (64, 64))])    # 16-byte and 4-byte ring rows
@pytest.mark.parametrize("scale", [1, 0.25])
def test_ring_rows_equal_the_reference_store_after_wrapping(O, A, hid, scale):
    import plugin
    from synth_tensor_humanoid import SynthTensorHumanoid

    N, S, cap, B = 16, 48, 200, 64
    kw = hip_kwargs(O, A, hid, B, buffer_max_size=cap, seed=5, sample_batch_size=S, reward_scale=scale, strict_rng=False)
    torch.manual_seed(1)
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    e = alg.engine
    assert buf.engine is e and cap % S

    class Env(SynthTensorHumanoid):        # the fixture's dynamics at this policy's shapes
        def reset(self, mask=None):
            return super().reset(mask)[:, :O].contiguous()

        def step(self, a):
            pad = torch.zeros(a.shape[0], 17 - a.shape[1], device=a.device)
            o2, r, te, tr = super().step(torch.cat([a, pad], dim=1))
            return o2[:, :O].contiguous(), r, te, tr

    env = Env(N, device="cuda", seed=4, episode_limit=torch.tensor([5, 1000] * (N // 2)))
    env.action_low, env.action_high = env.action_low[:A], env.action_high[:A]
    smp = plugin.create_sampler(sampler_name="hip_tensor_env_sampler", env=env, networks=alg.networks, **kw)
    ref = _HostRing(cap, O, A)
    seen_trunc = seen_term = False
    for rnd in range(6):                    # 288 transitions into 200 rows
        batch, _ = smp.sample()
        e.sync()
        host = [t.cpu().numpy() for t in batch.device_columns]
        buf.add_batch(batch)
        obs, act, rew, obs2, term, trunc, logp = host
        seen_trunc, seen_term = seen_trunc or bool(trunc.any()), seen_term or bool((term & ~trunc).any())
        for i in range(S):
            ref.store(obs[i], act[i], scale * float(rew[i]), obs2[i], bool(term[i]) and not bool(trunc[i]), logp[i])
        assert (buf.ptr, buf.size) == (ref.ptr, ref.size), rnd
        assert e.debug_get("ring_commit_rows") == (rnd + 1) * S
    for r0 in range(0, cap, B):
        rows = np.arange(r0, r0 + B) % cap
        e.gather(rows)
        got = e.read_batch(with_logp=True)
        for k in ("obs", "act", "rew", "obs2", "done", "logp"):
            w = ref.buf[k][rows]
            assert np.array_equal(np.asarray(got[k]).reshape(B, -1).view(np.uint32), w.reshape(B, -1).view(np.uint32)), (k, r0)
    assert seen_trunc                          # time-outs were among the transitions (stored as non-terminal)
    assert e.debug_get("act_dev_syncs") == 0.0


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def test_a_sample_makes_no_host_round_trip():
    import plugin
    from synth_tensor_humanoid import SynthTensorHumanoid

    O, A, N, S = 376, 17, 2048, 4096
    kw = hip_kwargs(O, A, (256, 256, 256), 256, buffer_max_size=10000, seed=5, sample_batch_size=S, strict_rng=False)
    torch.manual_seed(1)
    alg = plugin.create_alg(**kw)
    buf = plugin.create_buffer(**kw)
    e = alg.engine
    smp = plugin.create_sampler(sampler_name="hip_tensor_env_sampler", env=SynthTensorHumanoid(N, device="cuda", seed=4),
                                networks=alg.networks, **kw)
    before = {k: e.debug_get(k) for k in ("act_batch_calls", "act_mode_calls", "act_host_calls", "act_copies")}
    batch, _ = smp.sample()
    buf.add_batch(batch)
    assert e.debug_get("act_dev_syncs") == 0.0
    assert e.debug_get("act_dev_calls") == (S // N) * 2           # 2048 rows: two chunks per lockstep step
    assert e.debug_get("ring_commit_rows") == S and buf.size == S
    for k, v in before.items():
        assert e.debug_get(k) == v, k
    assert all(t.is_cuda for t in batch.device_columns) and batch._tuples is None and len(batch) == S
    e.sync()
    a = batch.act.cpu().numpy()
    assert np.isfinite(a).all() and np.abs(a).max() <= 0.4 and len({tuple(r) for r in a[:64].round(6)}) == 64
    first = batch[0]                                              # code that walks the reference's tuples still works
    assert np.array_equal(first[2], a[0]) and first[0].shape == (O,)


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
def test_serial_trainer_runs_with_the_sampler(tmp_path, K):
    import plugin
    from synth_tensor_humanoid import SynthTensorHumanoid
    from training.hip_trainer import HipOffSerialTrainer, read_scalars

    O, A, N, S, iters, cap, warm = 376, 17, 64, 128, 320, 5000, 256
    finals = []
    for run in range(2):
        folder = str(tmp_path / ("run%d" % run))
        kw = hip_kwargs(O, A, (256, 256, 256), 256, buffer_max_size=cap, buffer_warm_size=warm, seed=3, sample_batch_size=S,
                        sample_interval=K, max_iteration=iters, log_save_interval=40, apprfunc_save_interval=100000,
                        eval_interval=100000, save_folder=folder, ini_network_dir=None, strict_rng=False, hip_device_indices=True,
                        reward_scale=0.25, sampler_name="hip_tensor_env_sampler")
        torch.manual_seed(kw["seed"]); np.random.seed(kw["seed"])
        alg = plugin.create_alg(**kw)
        buf = plugin.create_buffer(**kw)
        smp = plugin.create_sampler(env=SynthTensorHumanoid(N, device="cuda", seed=4, episode_limit=50), **kw)
        tr = plugin.create_trainer(alg, smp, buf, None, **kw)
        assert type(tr) is HipOffSerialTrainer
        tr.train()
        e = alg.engine
        e.sync()
        n_samples = warm // S * S + (iters + K - 1) // K * S
        assert smp.get_total_sample_number() == n_samples and smp.act_step == n_samples // N
        assert buf.size == min(n_samples, cap) and buf.ptr == n_samples % cap and buf.index_iteration == iters
        assert e.debug_get("handoff_failures") == 0.0 and e.debug_get("act_dev_syncs") == 0.0
        assert e.debug_get("ring_commit_rows") == n_samples and e.debug_get("act_batch_calls") == 0.0
        scal = read_scalars(folder)
        assert len(scal["Loss/Critic loss-RL iter"]["y"]) == iters // 40
        for tag, d in scal.items():
            assert np.isfinite(d["y"]).all(), tag
        assert torch.isfinite(e.online).all()
        finals.append((e.online.cpu().clone(), e.target.cpu().clone(), e.adam_m.cpu().clone()))
    for x, y in zip(*finals):
        assert torch.equal(x, y)


# ---- 9 -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from dsact._ffi import DsactError

    O, A = 17, 6
    alg, _ = make_pair(O, A, (64, 64), 64, seed=4)
    e = alg.engine
    e.buffer_create(100)
    n = 8
    f = lambda *s: torch.zeros(*s, device="cuda")
    obs, act, clip, lp = f(n, O), f(n, A), f(n, A), f(n)
    flags = torch.zeros(n, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(DsactError, match="E_STATE.*dsact_set_act_rng"):
        e.act_sample_device(obs, None, 0, act, clip, lp)           # eps == NULL without a seed
    # host pointers (pageable and pinned) at the C-ABI itself: the Python wrapper would refuse them first
    h_obs, h_out = np.zeros((n, O), np.float32), np.zeros((n, A), np.float32)
    pinned = torch.zeros(n, O).pin_memory()
    P = lambda t: C.c_void_p(t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr())
    lib, h = e._lib, e._h
    e.set_act_rng(9)
    for bad_obs in (h_obs, pinned):
        assert lib.dsact_act_sample_device(h, P(bad_obs), n, None, 0, P(act), P(clip), P(lp)) == -1
        assert b"device pointers" in lib.dsact_last_error(h)
    assert lib.dsact_act_sample_device(h, P(obs), n, None, 0, P(h_out), P(clip), P(lp)) == -1
    assert lib.dsact_buffer_add_device(h, n, P(h_obs), P(act), P(lp), P(obs), P(flags), P(flags), P(lp), 1.0) == -1
    assert b"device pointers" in lib.dsact_last_error(h) and e.buffer_size == 0
    with pytest.raises(ValueError, match="obs must be a torch tensor on"):
        e.act_sample_device(torch.zeros(n, O), None, 0, act, clip, lp)
    with pytest.raises(ValueError, match="dtype"):
        e.act_sample_device(obs.double(), None, 0, act, clip, lp)
    with pytest.raises(ValueError, match="contiguous"):
        e.act_sample_device(f(O, n).t(), None, 0, act, clip, lp)
    with pytest.raises(DsactError, match="exceeds the capacity"):
        e.buffer_add_device(f(101, O), f(101, A), f(101), f(101, O), torch.zeros(101, dtype=torch.bool, device="cuda"),
                            torch.zeros(101, dtype=torch.bool, device="cuda"), f(101))
    # ... and the handle works
    e.act_sample_device(obs, None, 0, act, clip, lp)
    e.buffer_add_device(obs, act, lp, obs, flags, flags, lp, 0.5)
    e.sync()
    assert e.buffer_size == n and e.buffer_ptr == n and torch.isfinite(act).all() and e.debug_get("act_dev_syncs") == 0.0


@pytest.mark.parametrize("coded", [False, True])
def test_cnn_handles_and_coded_rings_are_refused(coded):
    from dsact._ffi import DsactError
    from test_coded_image_ring import BOOK
    from test_hip_groups import _family_alg

    B, n, O, A = 16, 4, 3 * 96 * 96, 3
    e = _family_alg("v2_cnn", B, seed=4)[0].engine
    e.buffer_create(32, codebook=BOOK if coded else None)
    f = lambda *s: torch.zeros(*s, device="cuda")
    obs, act, lp, flags = f(n, O), f(n, A), f(n), torch.zeros(n, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    e.set_act_rng(5)
    with pytest.raises(DsactError, match="E_INVALID.*serves MLP policies"):
        e.act_sample_device(obs, None, 0, act, f(n, A), lp)
    with pytest.raises(DsactError, match="E_INVALID.*coded rings" if coded else "E_INVALID.*image rings"):
        e.buffer_add_device(obs, act, lp, obs, flags, flags, lp)
    assert e.buffer_size == 0
    # the handle's own routes still work
    g = torch.Generator(device="cuda").manual_seed(9)
    book = torch.as_tensor(BOOK, device="cuda")
    img = book[torch.randint(0, 256, (n, O), device="cuda", generator=g)].contiguous()
    e.buffer_fill_device(0, img, act, lp, img, lp)
    assert e.buffer_size == n
    a = e.act_mode_batch(img.cpu().numpy())
    assert a.shape == (n, A) and np.isfinite(a).all()
