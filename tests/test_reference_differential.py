"""Differential tests against the reference: what the unmodified reference's own sampler,
evaluator, replay buffer, action distribution and CSV export produced (recorded by oracle/reference_vectors.py, in
tests/golden/oracle_vs_reference.npz) against the HIP host layer. No GPU and no reference checkout is needed -- the acting path
of a CPU container is torch.

  * the reference `OffSampler(algorithm="DSAC_V2_HIP")` found `dsac_v2_hip.ApproxContainer` by its own discovery rule
    (training/off_sampler.py:19-23); `HipOffSampler` produces its transitions from the same weights and seeds
  * the discovery rule as plugin.py restates it resolves the HIP module and class names; without a GPU construction fails
    LOUDLY in the HIP layer (no silent CPU fallback)
  * the reference `ReplayBuffer` and the host mirror of the HIP ring agree on ptr/size/sample indices
"""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import hip_kwargs

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "dsac-v2_amd")
for _p in (PKG, os.path.join(HERE, "envs")):
    if _p not in sys.path:
        sys.path.append(_p)


def sampler_kwargs(**over):
    kw = hip_kwargs(3, 1, (32, 32), 16, act_limit=2.0, env_id="synth_pendulum", sample_batch_size=25,
                    batch_size_per_sampler=25, noise_params=None, reward_scale=1, seed=11, max_episode_steps=60)
    kw.update(over)
    return kw


def _recorded_container(gold, part, **kw):
    import dsac_v2_hip

    c = dsac_v2_hip.ApproxContainer(**kw)
    sd = c.state_dict()
    c.load_state_dict({k: torch.as_tensor(gold(part, "init/" + k)) for k in sd})
    return c


def test_reference_sampler_with_hip_container_equals_hip_sampler():
    """the reference's `OffSampler(algorithm="DSAC_V2_HIP")` (training/off_sampler.py:19-97: it found
    `dsac_v2_hip.ApproxContainer` by its own discovery rule) recorded its initial weights, first observation and 150
    transitions from the seeds below; `HipOffSampler` acting with the same weights in the same environment must produce them,
    transition for transition (oracle/reference_vectors.py::record_loop_parts)."""
    import plugin
    from oracle import reference_vectors as rv
    from training.hip_sampler import HipOffSampler

    gold = rv.load()
    kw = rv.sampler_kwargs(hip_kwargs)
    env = plugin.create_env(**kw)                       # the wrapper stack the reference sampler acts in
    env.seed(kw["seed"])
    hip_s = HipOffSampler(env=env, **kw)
    hip_s.networks = _recorded_container(gold, "sampler", **kw)
    np.testing.assert_array_equal(np.asarray(hip_s.obs, np.float64), gold("sampler", "first_obs"))
    got = {}
    rv.sampler_calls(hip_s, got)
    assert str(got.pop("sampler/act_dtype")) == str(gold("sampler", "act_dtype"))
    for k, v in got.items():
        want = gold("sampler", k[len("sampler/"):])
        if k in ("sampler/done", "sampler/truncated", "sampler/total"):
            np.testing.assert_array_equal(v, want, err_msg=k)
        else:   # same torch build on the same kind of host => bit-exact; elsewhere the last ulps may differ
            np.testing.assert_allclose(v, want, rtol=1e-6, atol=1e-6, err_msg=k)
    assert int(got["sampler/truncated"].sum()) == 2 and float(got["sampler/total"]) == 150


def test_reference_factories_resolve_the_hip_modules():
    """the reference's discovery rule (utils/initialization.py:48-110: module algorithm.lower(), class algorithm; "training." +
    buffer_name.lower(), class CamelCase(buffer_name)) as plugin.py restates it resolves the HIP modules, and without a GPU
    construction fails LOUDLY in the HIP layer (no silent CPU fallback)"""
    if torch.cuda.is_available():
        pytest.skip("GPU present: construction succeeds")
    import importlib

    import plugin
    from dsact._ffi import DsactError

    plugin.install()
    kw = sampler_kwargs(buffer_max_size=256)
    with pytest.raises((DsactError, RuntimeError)) as ei:
        plugin.create_alg(**kw)
    assert "dsac_v2_hip" in "".join(str(f.path) for f in ei.traceback)
    mod = importlib.import_module("training." + kw["buffer_name"])
    assert mod.__file__.startswith(PKG) and hasattr(mod, "HipReplayBuffer")
    with pytest.raises((DsactError, RuntimeError)) as ei:
        plugin.create_buffer(**kw)
    assert "hip_replay_buffer" in "".join(str(f.path) for f in ei.traceback)
    with pytest.raises((DsactError, RuntimeError)) as ei:
        plugin.create_alg(**dict(kw, algorithm="DSAC_V1_HIP", TD_bound=10))
    assert "dsac_v1_hip" in "".join(str(f.path) for f in ei.traceback)


def test_reference_replay_buffer_vs_host_mirror():
    """reference ReplayBuffer (training/replay_buffer.py:20-90, its recorded vectors) vs oracle ReplayOracle, which the GPU tests
    compare the HIP ring against bit for bit (tests/test_hip_parity.py::test_replay_ring_and_gather_bit_exact): ptr / size after
    every add_batch, and the sampled rows after the same np.random.seed."""
    from oracle import reference_vectors as rv
    from oracle.dsact_oracle import ReplayOracle

    gold = rv.load()
    got = rv.replay_case(ReplayOracle)
    assert len(got) == 6 * 7
    for k, v in got.items():
        np.testing.assert_array_equal(v, gold("replay", k), err_msg=k)


def test_csv_export_equals_the_reference_export(tmp_path):
    """f3: after training the reference's scripts call save_tb_to_csv(save_folder) (utils/tensorboard_setup.py:121-139).
    The HIP trainer logs to scalars.jsonl; its export must produce the same files with the same bytes as the reference's own
    function produced from the same scalars (recorded by oracle/reference_vectors.py::record_loop_parts), and the tag
    dictionary must be the reference's."""
    import json

    from oracle import reference_vectors as rv
    from training.hip_trainer import TB_TAGS, _Scalars, save_tb_to_csv

    gold = rv.load()
    assert TB_TAGS == json.loads(str(gold("csv", "tb_tags")))
    want = json.loads(str(gold("csv", "files")))
    rv.csv_scalars(_Scalars, str(tmp_path), TB_TAGS)
    files = save_tb_to_csv(str(tmp_path))
    names = sorted(os.listdir(tmp_path / "data"))
    assert names == sorted(os.path.basename(f) for f in files) == sorted(want) and len(names) == 7
    assert "Time_Algorithm time [ms]-RL iter.csv" in names and "Evaluation_2. TAR-Total time [s].csv" in names
    for n in names:
        assert (tmp_path / "data" / n).read_bytes() == want[n].encode(), n


def test_reference_evaluator_with_hip_container_equals_hip_evaluator(tmp_path):
    """f3: the reference `Evaluator(algorithm="DSAC_V2_HIP")` (training/evaluator.py:9-84: mode() actions, episode return = sum
    of rewards, mean over num_eval_episode) recorded its weights and three evaluation returns; `HipEvaluator` on the same seeded
    environment with the same weights must return them, episode after episode."""
    import plugin
    from oracle import reference_vectors as rv
    from training.hip_trainer import HipEvaluator

    gold = rv.load()
    kw = rv.evaluator_kwargs(hip_kwargs, str(tmp_path))
    env = plugin.create_env(**dict(kw, reward_scale=None, repeat_num=None))     # what the reference evaluator builds (:12-14)
    hip_e = HipEvaluator(eval_env=env, **kw)
    hip_e.networks = _recorded_container(gold, "evaluator", **kw)
    got = [float(hip_e.run_evaluation(it)) for it in range(3)]
    np.testing.assert_allclose(got, gold("evaluator", "returns"), rtol=1e-6)
    assert all(np.isfinite(got)) and all(abs(a) > 1.0 for a in got)     # real returns, not empty episodes


def test_cpu_container_action_distribution_equals_the_reference():
    """VERDICT r2 (row a5): `dsac_v2_hip.TanhGaussDistribution` -- what a CPU `ApproxContainer` hands samplers and
    evaluators -- against what the reference's class (utils/act_distribution_cls.py:21-79) produced from the same logits,
    limits and generator state: sample / rsample (and how much of the global stream they consume), mode, log_prob, entropy."""
    import dsac_v2_hip
    from oracle import reference_vectors as rv

    gold = rv.load()
    got = rv.distribution_case(dsac_v2_hip.TanhGaussDistribution)
    for k, v in got.items():
        if k.endswith("next_draw"):     # the same amount of the global stream is consumed
            np.testing.assert_array_equal(v, gold("distribution", k), err_msg=k)
        else:    # same torch build on the same kind of host => bit-exact; elsewhere the last ulps may differ
            np.testing.assert_allclose(v, gold("distribution", k), rtol=1e-6, atol=1e-7, err_msg=k)
