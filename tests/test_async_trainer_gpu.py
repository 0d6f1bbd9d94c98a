"""HipOffAsyncTrainer on the whole HIP stack (DSAC_V2_HIP + HipReplayBuffer + the held behaviour policy, strict_rng) against
the CPU lagged serial restatement of tests/test_async_trainer_host.py (the oracle update and ring, the sampler acting with the
policy one group old): replay indices, ring size / ptr, the (tag, step) list of every scalar, checkpoint names and evaluation
iterations exactly; statistics, evaluation returns and logged values at the gates of the serial trainer's GPU trajectory test
(tests/test_trainer_trajectory.py). K = 2 and 8, with HipOffSampler and with HipVecOffSampler on its host and GPU routes.
"""
import pytest
import torch

from oracle.trainer_trajectory import TIME_TAGS, variant_case
from test_async_trainer_host import _async, _lagged_serial_cls, derived_kwargs, run_loop

pytestmark = pytest.mark.gpu

RAM_TAG = "RAM/RAM [MB]-RL iter"
SAMPLERS = {
    "single": {},
    "vec_host": dict(sampler_name="hip_vec_off_sampler", vector_env_num=4, hip_vec_act="host"),
    "vec_gpu": dict(sampler_name="hip_vec_off_sampler", vector_env_num=4, hip_vec_act="gpu"),
}


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("K", [2, 8])
def test_hip_stack_follows_the_lagged_serial_loop(tmp_path, K, sampler):
    import plugin
    from training.hip_async_trainer import HipOffAsyncTrainer

    case = dict(variant_case("si%d" % K), algorithm="DSAC_V2_HIP", **SAMPLERS[sampler])
    want, _ = run_loop(derived_kwargs(case, str(tmp_path / "cpu")), _lagged_serial_cls())

    kw = derived_kwargs(dict(case, buffer_name="hip_replay_buffer"), str(tmp_path / "hip"), strict_rng=True)
    alg = plugin.create_alg(**kw)
    buffer = plugin.create_buffer(**kw)
    assert buffer.engine is alg.engine
    got, tr = run_loop(kw, _async, alg=alg, buffer=buffer)
    e = alg.engine
    assert type(tr) is HipOffAsyncTrainer
    if sampler != "single":
        assert tr.sampler.route() == sampler[4:]
    # every group start held the behaviour policy, every sampler call after S_0 acted with it; nothing is held afterwards
    assert e.debug_get("beh_holds") == -(-case["max_iteration"] // K)
    assert e.debug_get("beh_acts") > 0 and e.debug_get("beh_held") == 0.0
    assert e.debug_get("handoff_failures") == 0.0

    for k in ("indices", "buffer", "saved", "apprfunc_dir", "warm", "samples"):
        assert got[k] == want[k], k
    assert [e_[0] for e_ in got["evals"]] == [e_[0] for e_ in want["evals"]]
    assert [t[:2] for t in got["tb"]] == [t[:2] for t in want["tb"]]
    assert any(t[1] >= 2 for t in got["tb"])
    crit = 7   # Loss/Critic loss: a sum of squared TD terms -> relative gate
    for g, w in zip(got["tb"], want["tb"]):
        for k, (a, b) in enumerate(zip(g[2:], w[2:])):
            tol = 1e-6 + 1e-5 * abs(b) if k == crit else 1e-4
            assert abs(a - b) <= tol, (g[:2], k, a, b)
    for (i0, a), (i1, b) in zip(got["evals"], want["evals"]):
        assert i0 == i1 and abs(a - b) <= 1e-4 * abs(b), (i0, a, b)
    wall = "Evaluation/2. TAR-Total time [s]"
    assert len(got["scalars"]) == len(want["scalars"])
    for g, w in zip(got["scalars"], want["scalars"]):
        assert g[0] == w[0] and (g[0] == wall or g[1] == w[1]), (g, w)
        if g[0] in TIME_TAGS or g[0] == RAM_TAG:
            continue
        assert abs(g[2] - w[2]) <= 1e-4 * max(1.0, abs(w[2])), (g, w)
    torch.cuda.synchronize()
