"""CNN acting path off the GPU: the opt-in's routing. The overlapped trainer accepts a CNN engine only
with `hip_cnn_act` in its kwargs AND an engine whose CNN acting path is enabled, and reads the engine's attribute only when the
kwarg is set; the samplers leave today's routes alone without the kwarg; the public header declares the export."""
import os
import re
import types

import pytest

from oracle.trainer_trajectory import TRAINER_CASE
from test_async_trainer_host import _Untouchable, derived_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _CnnEngine:
    """a CNN engine off the GPU: every attribute the refusal path is not allowed to read fails the test (`touched` lists what
    was read beyond conv_type); cnn_act exists only where a case sets it"""

    def __init__(self, **attrs):
        self.__dict__["_attrs"] = dict(conv_type="type_2", batch=64, comm_world=1, cfg=types.SimpleNamespace(global_batch=64), **attrs)
        self.__dict__["touched"] = []

    def __getattr__(self, k):
        if k in ("behaviour_hold", "behaviour_release"):
            return self._call
        if k in self._attrs:
            if k != "conv_type":
                self.touched.append(k)
            return self._attrs[k]
        raise AssertionError("engine attribute %s read before the refusal" % k)

    def _call(self, *a, **k):
        raise AssertionError("engine call before the refusal")


class _Alg:
    def __init__(self, networks, engine):
        self.networks, self.engine = networks, engine

    def hold_behaviour(self):
        raise AssertionError("hold before the refusal")

    release_behaviour = hold_behaviour


class HipCnnStochaPolicy:
    """a stand-in carrying the class name the routes look for and an engine"""

    def __init__(self, engine):
        self._engine = engine

    def parameters(self):
        return []


def _refused(tmp_path, engine, sampler_kw=None, **trainer_kw):
    import plugin
    from training.hip_async_trainer import HipOffAsyncTrainer

    kw = derived_kwargs(dict(TRAINER_CASE, algorithm="DSAC_V2_HIP"), str(tmp_path))
    sampler = plugin.create_sampler(**dict(kw, **(sampler_kw or {})))
    sampler.sample = lambda: (_ for _ in ()).throw(AssertionError("sampled before the refusal"))
    alg = _Alg(sampler.networks, engine)
    with pytest.raises(NotImplementedError) as ex:
        HipOffAsyncTrainer(alg, sampler, _Untouchable(), _Untouchable(), **dict(kw, trainer="hip_off_async_trainer", **trainer_kw))
    return str(ex.value)


def test_trainer_without_the_kwarg_refuses_a_cnn_engine_and_reads_nothing_new(tmp_path):
    eng = _CnnEngine()            # no cnn_act attribute at all: reading it would fail the test
    msg = _refused(tmp_path, eng)
    assert "CNN" in msg and eng.touched == []


def test_trainer_with_the_kwarg_refuses_an_engine_that_was_not_enabled(tmp_path):
    eng = _CnnEngine(cnn_act=False)
    msg = _refused(tmp_path, eng, hip_cnn_act=True)
    assert "hip_cnn_act" in msg and eng.touched == ["cnn_act"]


def test_trainer_with_an_enabled_engine_still_refuses_the_module_route(tmp_path):
    eng = _CnnEngine(cnn_act=True)
    # (the sampler's own container is an unattached MLP one: the vectorised sampler acts through the module forward)
    msg = _refused(tmp_path, eng, sampler_kw=dict(sampler_name="hip_vec_off_sampler", vector_env_num=4, hip_cnn_act=True),
                   hip_cnn_act=True)
    assert "module forward" in msg
    # ... and a one-environment sampler that does not reach the engine through dsact_act_sample is refused as well
    assert "dsact_act_sample" in _refused(tmp_path, _CnnEngine(cnn_act=True), hip_cnn_act=True)


def _stub_engine(cnn_act):
    return types.SimpleNamespace(conv_type="type_2", cnn_act=cnn_act, obs_dim=3 * 96 * 96, act_dim=3,
                                 debug_get=lambda name: 1.0 if cnn_act else 0.0)


@pytest.mark.parametrize("vec_act", ["auto", "gpu", "host"], ids=["act_auto", "act_gpu", "act_host"])
def test_vec_sampler_routes(tmp_path, vec_act):
    import plugin

    kw = derived_kwargs(dict(TRAINER_CASE, algorithm="DSAC_V2_HIP"), str(tmp_path))
    base = dict(kw, sampler_name="hip_vec_off_sampler", vector_env_num=4, hip_vec_act=vec_act)
    nets = types.SimpleNamespace(policy=HipCnnStochaPolicy(_stub_engine(True)))
    off = plugin.create_sampler(**base)
    off.networks = nets
    assert off.route() == "module"                       # without the kwarg: today's route
    on = plugin.create_sampler(**dict(base, hip_cnn_act=True))
    on.networks = nets
    assert on.route() == "gpu"                           # whatever hip_vec_act / hip_vec_gpu_min_envs say
    on.networks = types.SimpleNamespace(policy=HipCnnStochaPolicy(_stub_engine(False)))
    assert on.route() == "module"                        # the engine was not enabled
    one = plugin.create_sampler(**dict(base, vector_env_num=1, hip_cnn_act=True))
    assert one.route() == "single"                       # N = 1 stays the wrapped HipOffSampler


def test_off_sampler_fast_engine(tmp_path):
    import plugin

    kw = derived_kwargs(dict(TRAINER_CASE, algorithm="DSAC_V2_HIP"), str(tmp_path))
    eng = _stub_engine(True)
    nets = types.SimpleNamespace(policy=HipCnnStochaPolicy(eng))
    off = plugin.create_sampler(**kw)
    off.networks = nets
    assert off._fast_engine() is None and off.per_row_engine() is None
    on = plugin.create_sampler(**dict(kw, hip_cnn_act=True))
    on.networks = nets
    assert on._fast_engine() is eng and on.per_row_engine() is eng
    on.networks = types.SimpleNamespace(policy=HipCnnStochaPolicy(_stub_engine(False)))
    assert on._fast_engine() is None


def test_header_declares_the_export():
    text = open(os.path.join(ROOT, "include", "dsact.h")).read()
    assert re.search(r"^int\s+dsact_cnn_acting_enable\s*\(\s*dsact_handle\s*\*\s*h\s*\)\s*;", text, re.M)
    from dsact import _ffi

    assert any(sym[0] == "dsact_cnn_acting_enable" for sym in _ffi.SYMBOLS)   # (tests/test_host_side.py holds the two lists together)
