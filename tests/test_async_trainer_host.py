"""HipOffAsyncTrainer (training/hip_async_trainer.py) on the CPU: the overlapped loop's semantics.

The trainer's contract: every host-visible operation in the serial trainer's order, except that the transitions S_{g+1} are
collected with the policy theta_g (one group old) instead of theta_{g+1}. Around the reference's arithmetic (the oracle update
and ring, restated here as tests/test_trainer_trajectory.py restates them, behind the group surface of DSAC_V2_HIP) it must
equal a LAGGED SERIAL restatement -- the serial loop whose sampler, at each group start, gets a copy of the policy taken one
group earlier -- exactly: replay indices, ring state, every scalar, checkpoint names and evaluation returns. And it must
differ from the serial trainer from S_1 on (the lag is real).
"""
import copy
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

from oracle.trainer_trajectory import ENVS, TIME_TAGS, TRAINER_CASE, Hooks, tb_floats, variant_case

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "dsac-v2_amd")
for _p in (PKG, ENVS):
    if _p not in sys.path:
        sys.path.append(_p)


def derived_kwargs(case, save_folder, **over):
    """what the reference's utils/init_args.py adds to the argument dict (shapes and limits from the env, bookkeeping keys,
    the global seeds)"""
    import plugin

    kw = dict(case, save_folder=save_folder, **over)
    env = plugin.create_env(**kw)
    kw["use_gpu"] = False
    kw["batch_size_per_sampler"] = kw["sample_batch_size"]
    kw["obsv_dim"] = env.observation_space.shape[0]
    kw["action_dim"] = env.action_space.shape[0]
    kw["action_high_limit"] = env.action_space.high.astype("float32")
    kw["action_low_limit"] = env.action_space.low.astype("float32")
    kw["additional_info"] = {}
    kw["cnn_shared"] = False
    os.makedirs(os.path.join(save_folder, "apprfunc"), exist_ok=True)
    seed = int(kw["seed"])
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return kw


class OracleAlg:
    """the reference's DSAC_V2 restated: dsac_v2_hip.ApproxContainer drawn from the torch generator in the reference's order, the
    oracle update behind it, `networks` following every update -- offered through DSAC_V2_HIP's group surface"""

    def __init__(self, kw):
        from dsac_v2_hip import ApproxContainer
        from oracle.dsact_oracle import TB_KEYS, DsactOracle, default_config

        self.networks = ApproxContainer(**kw)
        A = int(kw["action_dim"])
        cfg = default_config(kw["obsv_dim"], A, kw["value_hidden_sizes"], policy_hidden=list(kw["policy_hidden_sizes"]))
        cfg["act_high"], cfg["act_low"] = np.asarray(kw["action_high_limit"], np.float32), np.asarray(kw["action_low_limit"], np.float32)
        rng = torch.get_rng_state()
        self.orc = DsactOracle(cfg, state_dict=self.networks.state_dict())
        torch.set_rng_state(rng)
        self.act_dim, self.time_key = A, TB_KEYS[-1]

    def local_update(self, data, it):
        return self._update(data, it)

    def _update(self, data, it):
        from oracle.dsact_oracle import draw_noise

        tb = self.orc.local_update(data, draw_noise(int(data["obs"].shape[0]), self.act_dim), it)
        self.networks.load_state_dict(self.orc.state_dict())
        tb.setdefault(self.time_key, 0.0)
        return tb

    def local_update_group(self, group, it):
        tb = None
        for j, batch in enumerate(group):
            tb = self._update(batch, it + j)
        return tb


class OracleBuffer:
    """the reference ReplayBuffer (the oracle ring) with HipReplayBuffer's group draw"""

    def __init__(self, kw):
        from oracle.dsact_oracle import ReplayOracle

        self.r = ReplayOracle(int(kw["obsv_dim"]), int(kw["action_dim"]), int(kw["buffer_max_size"]))

    size = property(lambda self: self.r.size)
    ptr = property(lambda self: self.r.ptr)

    def add_batch(self, samples):
        self.r.add_batch(samples)

    def sample_batch(self, n):
        return self.r.sample_batch(n)

    def sample_batches(self, batch_size, n):
        return [self.r.sample_batch(batch_size) for _ in range(n)]

    def __get_RAM__(self):
        return 0.0


def _lagged_serial_cls():
    from training.hip_trainer import HipOffSerialTrainer

    class LaggedSerialTrainer(HipOffSerialTrainer):
        """the serial loop whose sampler, at each group start, acts with a copy of the policy taken one group earlier (at
        the first group: the live policy)"""

        def step(self):
            if self.iteration % self.sample_interval == 0:
                now = copy.deepcopy(self.networks)
                self.sampler.networks = getattr(self, "_one_group_ago", None) or now
                self._one_group_ago = now
            super().step()

    return LaggedSerialTrainer


def run_loop(kw, make_trainer, steps=None, alg=None, buffer=None):
    """(trajectory dict, trainer): the loop of `make_trainer` around the oracle alg / ring (or the given alg / buffer); steps:
    call step() that many times instead of train()"""
    import plugin

    if alg is None:
        alg, buffer = OracleAlg(kw), OracleBuffer(kw)
    sampler = plugin.create_sampler(**kw)
    evaluator = plugin.create_evaluator(**kw)
    adds, evals, buf_state, tbs = [], [], [], []
    inner_add, inner_eval, inner_batches, inner_batch = buffer.add_batch, evaluator.run_evaluation, buffer.sample_batches, buffer.sample_batch
    inner_group, inner_update = alg.local_update_group, alg.local_update

    def add_batch(samples):
        adds.append(np.array([np.concatenate([np.ravel(s[0]), np.ravel(s[2]), [s[3]]]) for s in samples], np.float32))
        inner_add(samples)

    def sample_batches(b, n):
        buf_state.append([int(buffer.size), int(buffer.ptr), n])
        return inner_batches(b, n)

    def sample_batch(b):
        buf_state.append([int(buffer.size), int(buffer.ptr), 1])
        return inner_batch(b)

    def local_update_group(group, it):
        tb = inner_group(group, it)
        tbs.append([int(it), len(group)] + tb_floats(tb))
        return tb

    def local_update(data, it):
        tb = inner_update(data, it)
        tbs.append([int(it), 1] + tb_floats(tb))
        return tb

    buffer.add_batch, buffer.sample_batches, buffer.sample_batch = add_batch, sample_batches, sample_batch
    alg.local_update_group, alg.local_update = local_update_group, local_update
    evaluator.run_evaluation = lambda it: (lambda r: (evals.append([int(it), float(r)]), r)[1])(inner_eval(it))
    with Hooks() as hk:
        trainer = make_trainer(alg, sampler, buffer, evaluator, **kw)
        warm = len(adds)
        if steps is None:
            trainer.train()
        else:
            for _ in range(steps):
                trainer.step()
                trainer.iteration += 1
            trainer.writer.flush()
    scalars = [[r["tag"], r["step"], r["value"]] for r in map(json.loads, open(os.path.join(kw["save_folder"], "scalars.jsonl")))]
    return {"indices": hk.indices, "buffer": buf_state, "saved": hk.saved, "evals": evals, "tb": tbs, "warm": warm,
            "adds": adds, "scalars": scalars, "apprfunc_dir": sorted(os.listdir(os.path.join(kw["save_folder"], "apprfunc"))),
            "samples": int(sampler.get_total_sample_number()),
            "ring": {k: v.copy() for k, v in buffer.r.buf.items()} if isinstance(buffer, OracleBuffer) else None}, trainer


def assert_same(got, want):
    """two runs of the same loop on the same arithmetic: everything equal (the wall-clock values excepted)"""
    for k in ("indices", "buffer", "saved", "evals", "tb", "warm", "apprfunc_dir", "samples"):
        assert got[k] == want[k], k
    assert len(got["adds"]) == len(want["adds"])
    for i, (a, b) in enumerate(zip(got["adds"], want["adds"])):
        np.testing.assert_array_equal(a, b, err_msg="add_batch %d" % i)
    for k in want["ring"]:
        np.testing.assert_array_equal(got["ring"][k], want["ring"][k], err_msg=k)
    assert len(got["scalars"]) == len(want["scalars"])
    wall = "Evaluation/2. TAR-Total time [s]"
    for g, w in zip(got["scalars"], want["scalars"]):
        assert g[0] == w[0] and (g[0] == wall or g[1] == w[1]), (g, w)
        if g[0] not in TIME_TAGS:
            assert g[2] == w[2], (g, w)


CASES = {"si1": TRAINER_CASE, "si2": variant_case("si2"), "si8": variant_case("si8"), "si8_sparse": variant_case("si8_sparse")}


def _async(*a, **k):
    import plugin

    return plugin.create_trainer(*a, **dict(k, trainer="hip_off_async_trainer"))


def _serial(*a, **k):
    import plugin

    return plugin.create_trainer(*a, **k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_async_trainer_equals_the_lagged_serial_loop(tmp_path, name):
    """K = 1, 2, 8 (dense events: a checkpoint at a group's last iteration -- 15 -- and logs / evaluations in mid-group) and 8
    with whole groups between events: the overlapped loop IS the lagged serial loop, to the last bit"""
    from training.hip_async_trainer import HipOffAsyncTrainer

    case = dict(CASES[name], algorithm="DSAC_V2_HIP")
    K = case["sample_interval"]
    got, tr = run_loop(derived_kwargs(case, str(tmp_path / "async")), _async)
    assert type(tr) is HipOffAsyncTrainer and tr.sampler.networks is tr.networks   # nothing held after train()
    want, _ = run_loop(derived_kwargs(case, str(tmp_path / "lagged")), _lagged_serial_cls())
    assert_same(got, want)
    if K > 1:
        assert any(t[1] >= 2 for t in got["tb"])   # the updates were issued as groups
    # ... and it is NOT the serial loop: S_0 is the same, every later batch was collected with a policy one group old
    serial, _ = run_loop(derived_kwargs(case, str(tmp_path / "serial")), _serial)
    assert serial["warm"] == got["warm"] and serial["samples"] == got["samples"] and len(serial["adds"]) == len(got["adds"])
    for i in range(got["warm"] + 1):
        np.testing.assert_array_equal(got["adds"][i], serial["adds"][i])
    s1 = got["warm"] + 1
    assert not np.array_equal(got["adds"][s1], serial["adds"][s1])
    assert serial["indices"] == got["indices"] and serial["saved"] == got["saved"]   # (index draws do not depend on the ring's contents)
    assert serial["tb"] != got["tb"]


def test_step_keeps_the_serial_behaviour(tmp_path):
    """step() called directly is the serial trainer's step (no lag, no hold); warm-up is unchanged"""
    case = dict(variant_case("si2"), algorithm="DSAC_V2_HIP")
    got, tr = run_loop(derived_kwargs(case, str(tmp_path / "async")), _async, steps=9)
    want, _ = run_loop(derived_kwargs(case, str(tmp_path / "serial")), _serial, steps=9)
    assert tr.sampler.networks is tr.networks
    assert_same(got, want)
    assert got["warm"] >= 1 and len(got["adds"]) == got["warm"] + 5


def test_create_trainer_selects_the_async_trainer_by_name_only(tmp_path):
    import plugin
    from training.hip_async_trainer import HipOffAsyncTrainer
    from training.hip_trainer import HipOffSerialTrainer

    kw = derived_kwargs(dict(TRAINER_CASE, algorithm="DSAC_V2_HIP", max_iteration=2, buffer_warm_size=20), str(tmp_path))
    alg, buffer = OracleAlg(kw), OracleBuffer(kw)
    for name, cls in ((None, HipOffSerialTrainer), ("off_serial_trainer", HipOffSerialTrainer), ("off_async_trainer", HipOffSerialTrainer),
                      ("off_sync_trainer", HipOffSerialTrainer), ("hip_off_async_trainer", HipOffAsyncTrainer)):
        k = dict(kw)
        k.pop("trainer", None)
        if name is not None:
            k["trainer"] = name
        t = plugin.create_trainer(alg, None, buffer, None, **k)
        assert type(t) is cls, name


class _NoGpu:
    """an engine-backed algorithm whose every engine call fails the test: the refusals come before anything runs"""

    class Engine:
        def __init__(self, conv_type=None, global_batch=64, comm_world=1):
            import types

            self.conv_type, self.batch, self.comm_world = conv_type, 64, comm_world
            self.cfg = types.SimpleNamespace(global_batch=global_batch)

        def __getattr__(self, k):
            if k in ("behaviour_hold", "behaviour_release"):
                return self._call
            raise AssertionError("engine call %s before the refusal" % k)

        def _call(self, *a, **k):
            raise AssertionError("engine call before the refusal")

    def __init__(self, networks, **eng):
        self.networks, self.engine = networks, self.Engine(**eng)

    def hold_behaviour(self):
        raise AssertionError("hold before the refusal")

    release_behaviour = hold_behaviour


class _Untouchable:
    def __getattr__(self, k):
        raise AssertionError("%s touched before the refusal" % k)


@pytest.mark.parametrize("setup", ["cnn", "global_batch", "comm_world", "vec_module", "general_path"])
def test_unsupported_setups_are_refused_before_anything_runs(tmp_path, setup):
    import plugin
    from training.hip_async_trainer import HipOffAsyncTrainer

    kw = derived_kwargs(dict(TRAINER_CASE, algorithm="DSAC_V2_HIP"), str(tmp_path))
    if setup == "vec_module":   # an unattached container: the vectorised sampler's module route (the live weights)
        sampler = plugin.create_sampler(**dict(kw, sampler_name="hip_vec_off_sampler", vector_env_num=4))
        assert sampler.route() == "module"
    else:
        sampler = plugin.create_sampler(**dict(kw, hip_sampler_general_path=(setup == "general_path")))
    inner = sampler.sample
    sampler.sample = lambda: (_ for _ in ()).throw(AssertionError("sampled before the refusal"))
    eng = {"cnn": dict(conv_type="type_2"), "global_batch": dict(global_batch=128), "comm_world": dict(comm_world=2)}.get(setup, {})
    alg = _NoGpu(sampler.networks, **eng)
    with pytest.raises(NotImplementedError):
        HipOffAsyncTrainer(alg, sampler, _Untouchable(), _Untouchable(), **dict(kw, trainer="hip_off_async_trainer"))
    with pytest.raises(NotImplementedError):
        plugin.create_trainer(alg, sampler, _Untouchable(), _Untouchable(), **dict(kw, trainer="hip_off_async_trainer"))
    assert inner is not None
