"""Exploration noise (`noise_params={"mean": ..., "std": ...}`; the reference's GaussNoise, training/off_sampler.py:32-36 and 58-65,
utils/explore_noise.py:17-23) -- the host side, without a GPU.

  a. the reference's own OffSampler with noise_params against HipOffSampler's general path: what the unmodified reference
     produced from the seeds below is recorded in tests/golden/explore_noise_reference.npz (`python tests/test_explore_noise_host.py
     --record` with DSACT_REFERENCE_ROOT set; the same driver serves the recording and the test). Where a reference checkout is
     named by DSACT_REFERENCE_ROOT the recording itself is checked against a live run first (in a child process: the loader puts
     stand-in modules into sys.modules);
  b. one vector draw per lockstep step equals N sequential draws, bit for bit; HipVecOffSampler's rows carry them;
  c. the parser and its refusals, before any environment or engine call, for all three samplers;
  d. HipTensorEnvSampler on a stub engine: one set_explore_noise call per engine, the run state;
  e. the word-level restatement of the in-kernel draw (Philox stream 6);
  f. a resumed HipOffSerialTrainer run with noise equals the uninterrupted one.
"""
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "dsac-v2_amd")
for _p in (ROOT, PKG, HERE, os.path.join(HERE, "envs")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from helpers import hip_kwargs   # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "explore_noise_reference.npz")
# the synthetic Pendulum has A = 1: "per_dim" is the array form of length A (NumPy makes the action float64 there)
CASES = {"shared": {"mean": 0.05, "std": 0.3}, "per_dim": {"mean": [0.05], "std": [0.3]}}
COLUMNS = ("obs", "act", "rew", "obs2", "done", "logp", "truncated")


def sampler_kwargs(**over):
    """tests/test_reference_differential.py's sampler case with a 10-step time limit: 25 transitions cross two resets. The
    plain Gaussian (with _exact_policy's std = 1) keeps log() out of logp: see _exact_policy"""
    kw = hip_kwargs(3, 1, (32, 32), 16, act_limit=2.0, env_id="synth_pendulum", sample_batch_size=25, batch_size_per_sampler=25,
                    noise_params=None, reward_scale=1, seed=11, max_episode_steps=10, policy_act_distribution="GaussDistribution")
    kw.update(over)
    return kw


def _drive(sampler, out, case):
    """one sample() call of 25 transitions after seeding both global generators -> out["<case>/<column>"], dtypes kept"""
    torch.manual_seed(100)
    np.random.seed(7)
    batch, _ = sampler.sample()
    rows = {k: [] for k in COLUMNS}
    for obs, info, act, rew, obs2, done, logp, info2 in batch:
        for k, v in (("obs", obs), ("act", act), ("rew", np.float64(rew)), ("obs2", obs2), ("done", bool(done)), ("logp", logp),
                     ("truncated", bool(info2["TimeLimit.truncated"]))):
            rows[k].append(np.asarray(v))
    for k, v in rows.items():
        assert len({a.dtype for a in v}) == 1, k
        out["%s/%s" % (case, k)] = np.stack(v)
    out["%s/next_draw" % case] = np.array([np.random.normal(), float(torch.randn(1))])   # where both generators stand afterwards


def _exact_policy(networks):
    """every weight matrix of the policy := one signed power of two per row, zeros elsewhere (the biases keep their random
    initialisation). A dot product then has ONE non-zero term, which is exact, so a layer's output is one correctly rounded
    add -- the same bits whatever BLAS kernel, summation order or thread count the host's torch build picks. The log-std
    half of the output layer is zero: std = exp(0) = 1 and ln(std) = 0 exactly in every implementation, so the plain Gaussian's
    logp is IEEE basic operations only. The recording can then be compared bit for bit on any host; with dense random weights
    the last bit of a layer follows the host's BLAS, and a tanh-Gaussian's logp the host's log() (torch takes it from a vendor
    library that answers differently, in the last bit, on another CPU vendor's hardware)."""
    rng = np.random.default_rng(0)
    params = list(networks.policy.named_parameters())
    with torch.no_grad():
        for _, p in params:
            if p.dim() == 2:
                w = np.zeros(tuple(p.shape), np.float32)
                cols = rng.permutation(max(p.shape))[:p.shape[0]] % p.shape[1]
                w[np.arange(p.shape[0]), cols] = rng.choice([0.5, 1.0, 2.0], p.shape[0]) * rng.choice([-1.0, 1.0], p.shape[0])
                p.copy_(torch.from_numpy(w))
        (_, w_out), (_, b_out) = params[-2], params[-1]      # the output layer: rows [A, 2A) are the log-std
        assert w_out.dim() == 2 and b_out.dim() == 1 and w_out.shape[0] == b_out.shape[0] == 2
        w_out[1:].zero_()
        b_out[1:].zero_()


def _drive_reference(out):
    """the unmodified reference's OffSampler (found `dsac_v2_hip.ApproxContainer` by its own discovery rule), per case"""
    from oracle import ref_loader

    ref_loader.import_reference()
    import plugin

    plugin.install()
    import training.off_sampler as ref_sampler_mod

    for case, params in CASES.items():
        torch.manual_seed(5)
        s = ref_sampler_mod.OffSampler(**sampler_kwargs(noise_params=params))
        _exact_policy(s.networks)
        for k, v in s.networks.state_dict().items():
            out["%s/init/%s" % (case, k)] = v.numpy().copy()
        out["%s/first_obs" % case] = np.asarray(s.obs)
        _drive(s, out, case)


class _ActionDtype:
    """the one wrapper of the reference's stack the bare synthetic environment lacks and noise makes visible: ConvertType
    (utils/wrapping_env.py) hands the environment the action in the action space's dtype -- float32, also when array noise
    parameters made the sampler's action (and its clip) float64"""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, k):
        return getattr(self.env, k)

    def step(self, a):
        return self.env.step(np.asarray(a).astype(self.env.action_space.dtype))


def _hip_case(gold, case, **over):
    import dsac_v2_hip
    import plugin
    from training.hip_sampler import HipOffSampler

    kw = sampler_kwargs(**dict(dict(noise_params=CASES[case], hip_sampler_general_path=True), **over))
    env = _ActionDtype(plugin.create_env(**kw))
    env.seed(kw["seed"])
    smp = HipOffSampler(env=env, **kw)
    nets = dsac_v2_hip.ApproxContainer(**kw)            # unattached: the module forward on the CPU
    nets.load_state_dict({k: torch.as_tensor(gold["%s/init/%s" % (case, k)]) for k in nets.state_dict()})
    smp.networks = nets
    return smp


# ---- a. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_general_path_equals_the_reference_sampler_with_noise(case, tmp_path):
    gold = dict(np.load(GOLDEN))
    root = os.environ.get("DSACT_REFERENCE_ROOT", "")
    if root and os.path.isfile(os.path.join(root, "dsac_v2.py")):   # a live reference: the recording is what it produces now
        live = str(tmp_path / "live.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--record", live], check=True, cwd=ROOT)
        now = np.load(live)
        assert sorted(now.files) == sorted(gold)
        for k in now.files:
            assert now[k].dtype == gold[k].dtype and np.array_equal(now[k], gold[k]), k
    smp = _hip_case(gold, case)
    assert np.array_equal(np.asarray(smp.obs), gold[case + "/first_obs"])
    got = {}
    _drive(smp, got, case)
    for k in COLUMNS + ("next_draw",):
        a, b = got["%s/%s" % (case, k)], gold["%s/%s" % (case, k)]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (case, k)     # bitwise, dtype included
    act = gold[case + "/act"]
    assert act.shape == (25, 1) and act.dtype == (np.float32 if case == "shared" else np.float64)
    assert int(gold[case + "/truncated"].sum()) == 2 and not gold[case + "/done"].any()        # two episode resets crossed
    assert (np.abs(act) > 2.0).any()                    # the tuple carries the un-clipped noised action, beyond the +-2 limits
    # the noise is there: without it the first action is another one
    plain = {}
    _drive(_hip_case(gold, case, noise_params=None), plain, case)
    assert not np.array_equal(plain[case + "/act"][0].astype(np.float64), act[0].astype(np.float64))
    assert np.array_equal(plain[case + "/logp"][0], gold[case + "/logp"][0])     # ... and logp is the un-noised sample's


# ---- b. one vector draw = N sequential draws ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean, std", [(0.05, 0.3), ([0.05, -0.1, 0.0], [0.3, 0.0, 1.5]), ([0.25], [0.5]), (0.1, [0.3, 0.2, 0.1])])
def test_a_vector_draw_equals_sequential_draws(mean, std):
    N = 5
    shape = np.shape(np.random.normal(mean, std))
    np.random.seed(123)
    seq = [np.random.normal(mean, std) for _ in range(N)]
    after_seq = np.random.normal()
    np.random.seed(123)
    vec = np.random.normal(mean, std, size=(N,) + shape)
    assert np.random.normal() == after_seq                       # the generator stands where the sequential draws leave it
    assert vec.dtype == np.float64 and vec.shape == (N,) + shape
    for i in range(N):
        assert np.array_equal(vec[i], np.asarray(seq[i])), i     # bit for bit
    assert type(seq[0]) is float if shape == () else seq[0].dtype == np.float64


@pytest.mark.parametrize("params", [{"mean": 0.05, "std": 0.3}, {"mean": [0.05], "std": [0.3]}], ids=["scalar", "array"])
def test_vec_sampler_with_one_environment_is_hip_off_sampler_with_noise(params):
    from plugin import create_sampler
    from training.hip_sampler import HipOffSampler

    kw = hip_kwargs(3, 1, (32, 32), 16, act_limit=2.0, env_id="synth_pendulum", sample_batch_size=20, seed=3, max_episode_steps=15,
                    noise_params=params)
    runs = []
    for make in (lambda: HipOffSampler(**kw), lambda: create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=1, **kw)):
        torch.manual_seed(0)
        smp = make()
        torch.manual_seed(1)
        np.random.seed(2)
        batches = [smp.sample()[0] for _ in range(2)]
        runs.append((batches, torch.randn(3), np.random.normal()))
    (b0, t0, n0), (b1, t1, n1) = runs
    assert torch.equal(t0, t1) and n0 == n1
    for x, y in zip(sum(b0, []), sum(b1, [])):
        assert x[2].dtype == y[2].dtype == (np.float32 if np.ndim(params["mean"]) == 0 else np.float64)
        for j in (0, 2, 4, 6):
            assert np.array_equal(x[j], y[j])
        assert x[3] == y[3] and x[5] == y[5] and x[7] == y[7]


@pytest.mark.parametrize("params", [{"mean": 0.05, "std": 0.3}, {"mean": [0.05], "std": [0.3]},
                                    {"mean": [0.05, -0.02], "std": [0.3, 0.0]}], ids=["scalar", "one", "per_dim"])
def test_module_route_rows_carry_the_sequential_draws(params):
    """N = 4 on the `module` route against a noise-free twin with the same seeds: in the first lockstep step (the same
    observations) row i is the twin's action plus the i-th sequential np.random.normal(mean, std), in NumPy's own arithmetic"""
    from plugin import create_sampler
    from test_vec_sampler_host import _VarEnv, _nets

    N, S = 4, 8
    out = []
    for p in (params, None):
        smp = create_sampler(sampler_name="hip_vec_off_sampler", envs=[_VarEnv(k) for k in range(N)], sample_batch_size=S,
                             networks=_nets(5, 2, 0.3), noise_params=p, action_dim=2)
        assert smp.route() == "module"
        torch.manual_seed(4)
        np.random.seed(9)
        seen = []
        for e in smp.envs:
            e.step = (lambda step: lambda a: (seen.append(np.array(a)), step(a))[1])(e.step)
        out.append((smp.sample()[0], seen, np.random.normal()))
    (noised, seen, after), (twin, _, _) = out
    np.random.seed(9)
    draws = [np.random.normal(params["mean"], params["std"]) for _ in range(N)]
    draws2 = [np.random.normal(params["mean"], params["std"]) for _ in range(N)]
    assert np.random.normal() == after                             # two lockstep steps: 2 N sequential draws' worth
    for i in range(N):
        want = twin[i][2] + draws[i]                               # (a scalar draw is a Python float: float32 arithmetic)
        assert noised[i][2].dtype == want.dtype and np.array_equal(noised[i][2], want), i
        assert np.array_equal(noised[i][6], twin[i][6])            # logp: the un-noised sample's
        assert np.array_equal(seen[i], np.clip(want, smp.low[i], smp.high[i])) and seen[i].dtype == want.dtype   # the environment: its clip
        assert np.array_equal(noised.packed[1][i], want.astype(np.float32))                            # the packed row: the fp32 cast
    assert any(np.abs(noised[i][2]).max() > 0.3 for i in range(N))
    # the second step's rows carry draws N .. 2N - 1: noised action - draw is a valid un-noised sample inside the limits
    for i in range(N):
        clean = np.asarray(noised[N + i][2], np.float64) - np.asarray(draws2[i], np.float64)
        assert np.abs(clean).max() <= 0.3 + 1e-6, i


# ---- c. the parser ------------------------------------------------------------------------------------------------------------------
def test_parser_shapes_and_refusals():
    from training.hip_acting_common import check_noise_dim, explore_noise, noise_shape

    assert explore_noise({}) is None and explore_noise({"noise_params": None}) is None
    m, s = np.array([0.1, 0.2, 0.3]), [0.5, 0.0, 1.0]
    got = explore_noise({"noise_params": {"mean": m, "std": s}, "action_dim": 3})
    assert got[0] is m and got[1] is s and got[2] is False and noise_shape(got) == (3,)      # the caller's own objects
    assert explore_noise({"noise_params": {"mean": 0.0, "std": 0.1}, "action_dim": 3})[2] is True
    assert explore_noise({"noise_params": {"mean": [0.0], "std": 0.1}, "action_dim": 3})[2] is True
    assert explore_noise({"noise_params": {"mean": 0.0, "std": [0.1, 0.2, 0.3]}, "action_dim": 3})[2] is False
    for params in ({"mean": 0}, {"std": 1.0}, {}, {"epsilon": 0.1, "action_num": 3}):
        with pytest.raises(NotImplementedError, match="exploration noise") as ei:
            explore_noise({"noise_params": params})
        for k in ("mean", "std"):
            assert (repr(k) in str(ei.value).split(";")[1]) == (k not in params), (params, k)       # the missing key is named
    for params in ({"mean": 0, "std": 1, "decay": 0.9}, {"mean": 0, "std": -0.1}, {"mean": 0, "std": float("nan")},
                   {"mean": 0, "std": float("inf")}, {"mean": float("nan"), "std": 1}, {"mean": [0, float("inf")], "std": 1},
                   {"mean": [0.0, 0.0], "std": [0.1, 0.1]}, {"mean": np.zeros((3, 1)), "std": 0.1}, {"mean": [0.0] * 3, "std": [-1, 0, 1]},
                   {"mean": [0.0, 0.0], "std": [0.1, 0.1, 0.1]}):
        with pytest.raises(ValueError):
            explore_noise({"noise_params": params, "action_dim": 3})
    for t in ("discret", "discrete"):
        with pytest.raises(NotImplementedError, match="continuous"):
            explore_noise({"noise_params": {"mean": 0, "std": 1}, "action_type": t})
    with pytest.raises(NotImplementedError):
        explore_noise({"noise_params": {"epsilon": 0.1, "action_num": 3}, "action_type": "discret"})
    late = explore_noise({"noise_params": {"mean": [0.0, 0.0], "std": 0.1}})     # no action_dim yet: checked when A is known
    check_noise_dim(late, 2)
    with pytest.raises(ValueError, match="neither 1 nor"):
        check_noise_dim(late, 3)


class NoEnv:
    num_envs, action_low, action_high = 8, torch.full((3,), -0.4), torch.full((3,), 0.4)

    def __getattr__(self, k):
        raise AssertionError("environment call %s before the refusal" % k)


class NoCalls:
    conv_type, obs_dim, act_dim, device = None, 5, 3, torch.device("cpu")
    act_low, act_high = np.full(3, -0.4, np.float32), np.full(3, 0.4, np.float32)

    def __getattr__(self, k):
        raise AssertionError("engine call %s before the refusal" % k)


BAD = [({"mean": 0}, NotImplementedError, "exploration noise"), ({"mean": 0, "std": 1, "x": 1}, ValueError, "exactly the keys"),
       ({"mean": 0, "std": -1}, ValueError, "std"), ({"mean": 0, "std": float("nan")}, ValueError, "std"),
       ({"mean": [0, 0], "std": 1}, ValueError, "neither 1 nor")]


@pytest.mark.parametrize("name", ["hip_off_sampler", "hip_vec_off_sampler", "hip_tensor_env_sampler"])
def test_refusals_come_before_any_environment_or_engine_call(name, monkeypatch):
    import plugin

    monkeypatch.setattr(plugin, "create_env", lambda **kw: (_ for _ in ()).throw(AssertionError("create_env before the refusal")))
    nets = types.SimpleNamespace(policy=types.SimpleNamespace(_engine=NoCalls()))
    base = dict(sampler_name=name, sample_batch_size=32, networks=nets, action_dim=3, action_type="continu")
    if name == "hip_vec_off_sampler":
        cases = [dict(base, envs=[NoEnv() for _ in range(4)]), dict(base, vector_env_num=4), dict(base, envs=[NoEnv()])]
    else:
        cases = [dict(base, env=NoEnv()), dict(base)]
    for kw in cases:
        for params, err, match in BAD:
            with pytest.raises(err, match=match):
                plugin.create_sampler(**dict(kw, noise_params=params))
        with pytest.raises(NotImplementedError, match="continuous"):
            plugin.create_sampler(**dict(kw, noise_params={"mean": 0, "std": 1}, action_type="discret"))
    if name == "hip_tensor_env_sampler":      # the length against the ENGINE's A when the kwargs carry none, still before any call
        kw = dict(base, env=NoEnv())
        kw.pop("action_dim")
        with pytest.raises(ValueError, match="neither 1 nor"):
            plugin.create_sampler(**dict(kw, noise_params={"mean": [0, 0], "std": 1}))
        with pytest.raises(ValueError, match="strict_rng"):
            plugin.create_sampler(**dict(kw, noise_params={"mean": 0, "std": 1}, strict_rng=True))


# ---- d. the tensor sampler on a stub engine ---------------------------------------------------------------------------------------
def _tensor_sampler(params, eng=None, **over):
    from plugin import create_sampler
    from synth_tensor_humanoid import SynthTensorHumanoid
    from test_tensor_sampler_host import FakeEngine, _networks

    class Engine(FakeEngine):
        def set_explore_noise(self, mean=None, std=None):
            self.calls.append(("set_explore_noise", mean, std))

        def sync(self):
            pass

    class Env(SynthTensorHumanoid):
        def state_dict(self):
            return {"pos": self.pos.clone(), "t": self.t.clone()}

        def load_state_dict(self, sd):
            self.pos, self.t = sd["pos"].clone(), sd["t"].clone()

    eng = eng or Engine()
    env = Env(8, seed=3)
    kw = dict(sampler_name="hip_tensor_env_sampler", env=env, sample_batch_size=16, networks=_networks(eng), seed=3, noise_params=params)
    kw.update(over)
    return create_sampler(**kw), eng


def test_tensor_sampler_sets_the_noise_once_per_engine():
    from test_tensor_sampler_host import A, _networks

    mean, std = np.linspace(-0.1, 0.1, A), np.full(A, 0.2)
    smp, eng = _tensor_sampler({"mean": mean, "std": std})
    for _ in range(3):
        smp.sample()
    sets = [c for c in eng.calls if c[0] == "set_explore_noise"]
    assert len(sets) == 1 and sets[0][1] is mean and sets[0][2] is std                  # one call, the parsed arrays
    names = [c[0] for c in eng.calls]
    assert names.index("set_act_rng") < names.index("set_explore_noise") < names.index("act_sample_device")
    eng2 = type(eng)()
    smp.networks = _networks(eng2)                                                       # a new engine: once more, there
    smp.sample()
    smp.sample()
    assert [c[0] for c in eng2.calls].count("set_explore_noise") == 1 and len([c for c in eng.calls if c[0] == "set_explore_noise"]) == 1
    # scalars: SHARED, handed over as they are
    smp3, eng3 = _tensor_sampler({"mean": 0.0, "std": 0.2})
    smp3.sample()
    assert [c[1:] for c in eng3.calls if c[0] == "set_explore_noise"] == [(0.0, 0.2)] and smp3.noise[2] is True
    # no noise_params: no call at all
    smp0, eng0 = _tensor_sampler(None)
    smp0.sample()
    smp0.sample()
    assert "set_explore_noise" not in [c[0] for c in eng0.calls] and smp0.noise is None
    # strict_rng stays refused
    with pytest.raises(ValueError, match="strict_rng"):
        _tensor_sampler({"mean": 0.0, "std": 0.2}, strict_rng=True)
    with pytest.raises(ValueError, match="neither 1 nor"):
        _tensor_sampler({"mean": [0.0, 0.1], "std": 0.2})


def test_tensor_sampler_run_state_carries_the_noise():
    from test_tensor_sampler_host import A

    params = {"mean": 0.0, "std": 0.2}
    smp, _ = _tensor_sampler(params)
    smp.sample()
    sd = pickle.loads(pickle.dumps(smp.run_state()))
    assert sd["explore_noise"] == ([0.0], [0.2], True)
    same, _ = _tensor_sampler(dict(params))
    same.load_run_state(sd)
    assert same.act_step == smp.act_step == 2
    for other in (None, {"mean": 0.0, "std": 0.3}, {"mean": 0.1, "std": 0.2}, {"mean": [0.0] * A, "std": [0.2] * A}):
        s2, _ = _tensor_sampler(other)
        with pytest.raises(ValueError, match="noise_params"):
            s2.load_run_state(sd)
        assert s2.act_step == 0
    # a state saved before the key existed means "no noise"
    plain, _ = _tensor_sampler(None)
    plain.sample()
    old = plain.run_state()
    assert old.pop("explore_noise") is None
    fresh, _ = _tensor_sampler(None)
    fresh.load_run_state(old)
    assert fresh.act_step == 2
    with pytest.raises(ValueError, match="noise_params"):
        _tensor_sampler(params)[0].load_run_state(old)
    per_dim, _ = _tensor_sampler({"mean": np.zeros(A), "std": np.full(A, 0.2)})
    assert per_dim.run_state()["explore_noise"] == ([0.0] * A, [0.2] * A, False)


# ---- e. the word-level restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act_dim", [1, 4, 6, 17])
def test_explore_noise_words_are_stream_six_and_shared_is_element_zero(act_dim):
    from test_device_indices_host import SEED, philox4x32_10
    from training.hip_tensor_sampler import (EXPLORE_STREAM, act_noise_reference, act_noise_words, explore_noise_reference,
                                             explore_noise_words)

    assert EXPLORE_STREAM == 6
    for step in (0, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7):
        for row in (0, 1, 1023, 1024):
            for d in sorted({0, act_dim // 2, act_dim - 1}):
                w, e = explore_noise_words(SEED, step, row, d, act_dim, False)
                s64 = step & ((1 << 64) - 1)
                want = philox4x32_10((row * -(-act_dim // 4) + d // 4, s64 & 0xFFFFFFFF, s64 >> 32, 6), (SEED & 0xFFFFFFFF, SEED >> 32))
                assert tuple(w) == tuple(want) and e == d % 4
                assert w != act_noise_words(SEED, step, row, d, act_dim)[0]                     # never eps's counter block
                assert explore_noise_words(SEED, step, row, d, act_dim, True) == explore_noise_words(SEED, step, row, 0, act_dim, False)
    z = explore_noise_reference(SEED, 7, 64, act_dim, False)
    zs = explore_noise_reference(SEED, 7, 64, act_dim, True)
    assert z.shape == zs.shape == (64, act_dim) and np.isfinite(z).all()
    assert (zs == zs[:, :1]).all() and np.array_equal(zs[:, 0], z[:, 0])                      # equal columns: the row's element 0
    assert np.array_equal(z[:4], explore_noise_reference(SEED, 7, 4, act_dim, False))         # independent of the number of rows
    assert not np.array_equal(z, act_noise_reference(SEED, 7, 64, act_dim))
    w = philox4x32_10((9 * -(-act_dim // 4), 7, 0, 6), (SEED & 0xFFFFFFFF, SEED >> 32))
    u0, u1 = ((w[0] >> 8) + 0.5) / 2 ** 24, ((w[1] >> 8) + 0.5) / 2 ** 24
    assert z[9, 0] == np.sqrt(-2 * np.log(u0)) * np.cos(2 * np.pi * u1)


def test_explore_noise_is_standard_normal():
    from test_device_indices_host import SEED
    from training.hip_tensor_sampler import explore_noise_reference

    z = np.concatenate([explore_noise_reference(SEED, s, 256, 17, False) for s in range(8)]).reshape(-1)
    assert abs(z.mean()) < 4 / np.sqrt(z.size) and abs(z.var() - 1) < 4 * np.sqrt(2 / z.size)


def test_the_symbol_is_declared_bound_and_exported():
    import ctypes as C
    import re

    from dsact import _ffi
    from dsact.engine import DsactEngine

    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    assert re.search(r"int dsact_set_explore_noise\(dsact_handle\* h, const float\* mean, const float\* std, int32_t n\);", hdr)
    doc = hdr[hdr.index("dsact_set_explore_noise(h, mean, std, n)"):hdr.index("int dsact_set_act_rng")]
    for cite in ("off_sampler.py:58-65", "explore_noise.py:17-23"):
        assert cite in doc, cite
    P = C.c_void_p
    assert {n: (r, a) for n, r, a in _ffi.SYMBOLS}["dsact_set_explore_noise"] == (C.c_int, [P, P, P, C.c_int32])
    lib = _ffi.load()
    assert lib.dsact_set_explore_noise(None, None, None, 0) == -1
    assert callable(DsactEngine.set_explore_noise)


# ---- f. a resumed run ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [{"mean": 0.05, "std": 0.3}, {"mean": [0.05], "std": [0.3]}], ids=["scalar", "array"])
def test_a_resumed_run_with_noise_equals_the_uninterrupted_one(tmp_path, params):
    """HipOffSerialTrainer's run state carries the global NumPy generator (run.pkl "numpy_rng"): the host samplers' noise needs
    nothing more. The ring after 12 iterations, interrupted after iteration 4 or not, is the same bytes."""
    from test_ring_snapshot_host import _parts
    from training.hip_trainer import HipOffSerialTrainer

    kw, alg, smp, buf, ev = _parts(tmp_path, "a", hip_save_run_state=True, hip_run_state_keep=8, noise_params=params)
    assert smp.noise is not None
    HipOffSerialTrainer(alg, smp, buf, ev, **kw).train()
    d = str(tmp_path / "a" / "apprfunc" / "run_state_4")
    kw2, alg2, smp2, buf2, ev2 = _parts(tmp_path, "b", ini_run_state_dir=d, noise_params=params)
    torch.manual_seed(77)
    np.random.seed(77)                                             # whatever was drawn before: the saved states come last
    tr2 = HipOffSerialTrainer(alg2, smp2, buf2, ev2, **kw2)
    assert tr2.iteration == 5
    tr2.train()
    assert buf.engine.state() == buf2.engine.state() and buf.size == 150
    assert smp.get_total_sample_number() == smp2.get_total_sample_number()
    assert np.array_equal(smp.obs, smp2.obs) and np.random.normal() is not None
    # ... and the noise reached the ring: a noise-free run stores other actions
    kw3, alg3, smp3, buf3, ev3 = _parts(tmp_path, "c", noise_params=None)
    HipOffSerialTrainer(alg3, smp3, buf3, ev3, **kw3).train()
    assert buf3.engine.state() != buf.engine.state()


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        recorded = {}
        _drive_reference(recorded)
        np.savez_compressed(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, **recorded)
        print("recorded %d arrays" % len(recorded))
