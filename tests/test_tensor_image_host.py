"""Device-resident image environments -- the host side, without a GPU:

  1. the three byte-frame entry points are declared in include/dsact.h, exported and bound;
  2. the sampler's gate: `hip_cnn_act=True` AND `engine.cnn_act`, the kwarg read first; its buffers are [S, C, H, W] rows in the
     environment's dtype; the evaluator's gate is the same;
  3. a byte DeviceSampleBatch walks as float32 tuples through the codebook;
  4. tests/envs/synth_tensor_blob.py: SynthBlob's trajectory at N = 1, every pixel a codebook value, the two frame dtypes equal
     through the codebook, rows independent of N, state_dict round trip.
"""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "dsac-v2_amd")
for _p in (ROOT, PKG, os.path.join(HERE, "envs")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_tensor_sampler_host import FakeEngine, _networks   # noqa: E402

BOOK = np.float32(np.arange(256) / 255.0)
SHAPE, A = (3, 96, 96), 3
O = int(np.prod(SHAPE))


# ---- 1. the C-ABI ------------------------------------------------------------------------------------------------------------------
def test_byte_frame_symbols_are_declared_exported_and_bound():
    import ctypes as C

    from dsact import _ffi

    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    P = C.c_void_p
    want = {
        "dsact_act_sample_device_u8": (r"int dsact_act_sample_device_u8\(dsact_handle\* h, const uint8_t\* frames_dev, int32_t n, "
                                       r"const float\* eps_dev, int64_t step,\s+float\* action_dev, float\* clipped_dev, float\* logp_dev\);",
                                       [P, P, C.c_int32, P, C.c_int64, P, P, P]),
        "dsact_act_mode_device_u8": (r"int dsact_act_mode_device_u8\(dsact_handle\* h, const uint8_t\* frames_dev, int32_t n, "
                                     r"float\* action_dev\);", [P, P, C.c_int32, P]),
        "dsact_buffer_add_device_u8": (r"int dsact_buffer_add_device_u8\(dsact_handle\* h, int64_t n, const uint8_t\* obs, const float\* act, "
                                       r"const float\* rew, const uint8_t\* obs2,\s+const uint8_t\* terminated, const uint8_t\* truncated, "
                                       r"const float\* logp, double reward_scale\);", [P, C.c_int64, P, P, P, P, P, P, P, C.c_double]),
    }
    bound = {n: (res, args) for n, res, args in _ffi.SYMBOLS}
    for name, (decl, args) in want.items():
        assert re.search(decl, hdr), name
        assert bound[name] == (C.c_int, args), name
    lib = _ffi.load()
    for name in want:
        assert hasattr(lib, name), name
    assert lib.dsact_act_sample_device_u8(None, None, 1, None, 0, None, None, None) == -1
    assert lib.dsact_act_mode_device_u8(None, None, 1, None) == -1
    assert lib.dsact_buffer_add_device_u8(None, 1, None, None, None, None, None, None, None, 1.0) == -1


# ---- 2. the gate and the buffers ---------------------------------------------------------------------------------------------------
class FakeCnnEngine(FakeEngine):
    """FakeEngine as an enabled CNN engine: frames come as [n, C, H, W] rows of either dtype"""
    conv_type, cnn_act, obs_shape = "type_2", True, SHAPE

    def __init__(self):
        super().__init__(obs_dim=O, act_dim=A, limit=1.0)

    def act_sample_device(self, obs, eps, step, action, clipped, logp):
        n = obs.shape[0]
        assert eps is None and tuple(obs.shape) == (n,) + SHAPE and obs.is_contiguous()
        action.copy_(0.5 * torch.sin(0.37 * step + torch.arange(A, dtype=torch.float32))[None, :].expand(n, A))
        clipped.copy_(action)
        logp.fill_(float(step))
        self.calls.append(("act_sample_device", n, int(step), obs.dtype))

    def act_mode_device(self, obs, action):
        self.calls.append(("act_mode_device", obs.shape[0], obs.dtype, tuple(obs.shape[1:])))
        action.zero_()


class NoCalls(FakeCnnEngine):
    def __getattribute__(self, k):
        if k in ("act_sample_device", "act_mode_device", "set_act_rng", "buffer_add_device"):
            raise AssertionError("engine call %s before the refusal" % k)
        return super().__getattribute__(k)


class NoEnv:
    num_envs, action_low, action_high = 4, torch.full((A,), -1.0), torch.full((A,), 1.0)

    def __getattr__(self, k):
        raise AssertionError("environment call %s before the refusal" % k)


@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_sampler_accepts_an_enabled_cnn_engine_and_keeps_image_rows_in_the_frames_dtype(frames):
    from plugin import create_sampler
    from synth_tensor_blob import SynthTensorBlob
    from training.hip_replay_buffer import HipReplayBuffer

    N, S = 4, 8
    eng = FakeCnnEngine()
    env = SynthTensorBlob(N, seed=3, frames=frames)
    smp = create_sampler(sampler_name="hip_tensor_env_sampler", env=env, sample_batch_size=S, networks=_networks(eng), seed=3,
                         hip_cnn_act=True)
    batch, _ = smp.sample()
    dt = getattr(torch, frames)
    assert tuple(batch.obs.shape) == (S,) + SHAPE == tuple(batch.obs2.shape) and batch.obs.dtype == batch.obs2.dtype == dt
    acts = [c for c in eng.calls if c[0] == "act_sample_device"]
    assert eng.calls[0] == ("set_act_rng", smp.act_seed) and [c[1:] for c in acts] == [(N, 0, dt), (N, 1, dt)]
    # step-major, and the next step's frame of an environment that did not end is this step's obs2
    assert torch.equal(batch.obs[N:], batch.obs2[:N]) and not torch.equal(batch.obs[:N], batch.obs[N:])
    eng.codebook = BOOK
    buf = HipReplayBuffer(obsv_dim=SHAPE, action_dim=A, buffer_max_size=100, replay_batch_size=16, hip_engine=eng)
    eng.calls.clear()
    buf.add_batch(batch)
    assert eng.calls == [("buffer_add_device", S, 1.0)] and batch._tuples is None


def test_sampler_and_evaluator_refuse_cnn_engines_outside_the_gate():
    from plugin import create_sampler
    from training.hip_tensor_evaluator import HipTensorEnvEvaluator

    off = NoCalls()
    off.cnn_act = False
    base = dict(sampler_name="hip_tensor_env_sampler", env=NoEnv(), sample_batch_size=8)
    for kw in (dict(networks=_networks(NoCalls())),                              # the kwarg absent
               dict(networks=_networks(NoCalls()), hip_cnn_act=False),
               dict(networks=_networks(off), hip_cnn_act=True)):                 # the engine not enabled
        with pytest.raises(NotImplementedError, match="CNN.*hip_cnn_act"):
            create_sampler(**dict(base, **kw))
        with pytest.raises(NotImplementedError, match="CNN.*hip_cnn_act"):
            HipTensorEnvEvaluator(env=NoEnv(), **kw)
    # the kwarg is read first: a stub without the attribute is refused without being asked for it
    class Bare(FakeEngine):
        conv_type = "type_2"

        def __getattr__(self, k):
            raise AssertionError("attribute %s read" % k)

    with pytest.raises(NotImplementedError, match="CNN"):
        create_sampler(**dict(base, networks=_networks(Bare())))
    # networks assigned later (what the trainer does): refused at sample(), still before any call
    smp = create_sampler(**dict(base, networks=None, hip_cnn_act=True))
    smp.networks = _networks(off)
    with pytest.raises(NotImplementedError, match="hip_cnn_act"):
        smp.sample()


@pytest.mark.parametrize("frames", ["float32", "uint8"])
def test_evaluator_accepts_image_environments_of_either_dtype(frames):
    from synth_tensor_blob import SynthTensorBlob
    from training.hip_tensor_evaluator import HipTensorEnvEvaluator

    N, E = 2, 3
    eng = FakeCnnEngine()
    eng.eval_begin = lambda n, e: None
    eng.eval_commit = lambda rew, term, trunc, ended: ended.copy_(term | trunc)
    eng.eval_poll = lambda: 0
    eng.eval_read = lambda e: (np.zeros(e), np.zeros(e, np.int32))
    eng.note_torch_writes = lambda p: None
    ev = HipTensorEnvEvaluator(env=SynthTensorBlob(N, seed=1, frames=frames), networks=_networks(eng), num_eval_episode=E,
                               hip_cnn_act=True, hip_eval_poll_steps=2)
    ev.run_evaluation(0)
    modes = [c for c in eng.calls if c[0] == "act_mode_device"]
    assert modes == [("act_mode_device", N, getattr(torch, frames), SHAPE)] * 2


# ---- 3. byte batches walk as float32 tuples -------------------------------------------------------------------------------------------
def test_byte_batch_iterates_as_float32_tuples_through_the_codebook():
    from training.hip_tensor_sampler import DeviceSampleBatch

    S = 6
    g = torch.Generator().manual_seed(2)
    b, b2 = (torch.randint(0, 256, (S,) + SHAPE, generator=g, dtype=torch.uint8) for _ in range(2))
    act, rew, logp = torch.randn(S, A, generator=g), torch.randn(S, generator=g), torch.randn(S, generator=g)
    term = torch.tensor([0, 1, 0, 1, 0, 0], dtype=torch.bool)
    trunc = torch.tensor([0, 0, 1, 1, 0, 0], dtype=torch.bool)
    batch = DeviceSampleBatch(b, act, rew, b2, term, trunc, logp, reward_scale=0.25, codebook=BOOK)
    tuples = list(batch)
    assert len(tuples) == S and len(batch) == S
    for i, t in enumerate(tuples):
        assert t[0].dtype == np.float32 and t[0].shape == SHAPE
        assert np.array_equal(t[0], BOOK[b[i].numpy()]) and np.array_equal(t[4], BOOK[b2[i].numpy()])
        assert np.array_equal(t[2], act[i].numpy()) and t[3] == 0.25 * float(rew[i]) and t[6] == float(logp[i])
        assert t[5] == (bool(term[i]) and not bool(trunc[i])) and t[7]["TimeLimit.truncated"] == bool(trunc[i])
    # float32 image rows keep their values and shape; a byte batch without a codebook cannot be walked
    f = DeviceSampleBatch(torch.from_numpy(BOOK)[b.long()], act, rew, torch.from_numpy(BOOK)[b2.long()], term, trunc, logp)
    assert np.array_equal(f[3][0], tuples[3][0]) and np.array_equal(f[3][4], tuples[3][4])
    with pytest.raises(ValueError, match="codebook"):
        list(DeviceSampleBatch(b, act, rew, b2, term, trunc, logp))


# ---- 4. the fixture ------------------------------------------------------------------------------------------------------------------
def test_synth_tensor_blob_walks_synth_blobs_trajectory_at_n1():
    """same seed, same actions: SynthBlob's targets (read off the rewards and the square's position), its truncation after 20
    steps and its restart draw. The pixels differ by construction (codebook values here, 0.1 / 0.9 + U(0, 0.02) there): the
    square is compared as a mask."""
    from synth_blob_data import SynthBlob
    from synth_tensor_blob import SynthTensorBlob

    seed = 11
    ref, env = SynthBlob(seed=seed, act_dim=A), SynthTensorBlob(1, seed=seed, act_dim=A)
    o_ref, o = ref.reset()[0], env.reset()
    rng = np.random.default_rng(5)
    n_trunc = 0
    for t in range(47):
        assert np.array_equal(o_ref > 0.5, o[0].numpy() > 0.5), t
        a = rng.uniform(-1, 1, A).astype(np.float32)
        o_ref, r_ref, done, info = ref.step(a)
        o2, r, term, trunc = env.step(torch.from_numpy(a)[None])
        assert abs(float(r[0]) - r_ref) <= 1e-6 * max(1.0, abs(r_ref)), (t, float(r[0]), r_ref)
        assert not done and not bool(term[0]) and bool(trunc[0]) == info["TimeLimit.truncated"]
        assert np.array_equal(o_ref > 0.5, o2[0].numpy() > 0.5), t
        o = env.reset(term | trunc)
        if info["TimeLimit.truncated"]:
            n_trunc += 1
            o_ref = ref.reset()[0]
        else:
            assert torch.equal(o, o2)
    assert n_trunc == 2


def test_synth_tensor_blob_pixels_are_codebook_values_in_both_dtypes_and_rows_do_not_depend_on_n():
    from synth_tensor_blob import BOOK as ENV_BOOK, SynthTensorBlob

    assert np.array_equal(ENV_BOOK.view(np.uint32), BOOK.view(np.uint32))
    N = 6
    f, b, one = (SynthTensorBlob(N, seed=4, frames="float32"), SynthTensorBlob(N, seed=4, frames="uint8"),
                 SynthTensorBlob(1, seed=4, frames="uint8", env_offset=3))
    book = torch.from_numpy(BOOK)
    g = torch.Generator().manual_seed(1)
    of, ob, oo = f.reset(), b.reset(), one.reset()
    for t in range(25):
        assert of.dtype == torch.float32 and ob.dtype == torch.uint8 and tuple(of.shape) == tuple(ob.shape) == (N,) + SHAPE
        assert torch.equal(of.view(torch.int32), book[ob.long()].view(torch.int32)), t       # the two dtypes agree through BOOK
        assert torch.isin(of, book).all() and torch.equal(ob[3:4], oo)
        a = torch.rand(N, A, generator=g) * 2 - 1
        (of, rf, tf, uf), (ob, rb, tb, ub), (oo, ro, to, uo) = f.step(a), b.step(a), one.step(a[3:4])
        assert torch.equal(rf, rb) and torch.equal(uf, ub) and not bool(tf.any()) and rf.dtype == torch.float32 and uf.dtype == torch.bool
        assert torch.equal(rb[3:4], ro) and torch.equal(ub[3:4], uo) and bool(uf.all()) == (t % 20 == 19)
        of, ob, oo = f.reset(tf | uf), b.reset(tb | ub), one.reset(to | uo)
    assert len({int(c) for c in ob.unique()}) <= 12 and int(ob.max()) < 256


def test_synth_tensor_blob_state_dict_round_trips():
    from synth_tensor_blob import SynthTensorBlob

    N = 3
    env = SynthTensorBlob(N, seed=9, frames="uint8")
    env.reset()
    a = torch.full((N, A), 0.25)
    for _ in range(7):
        env.step(a)
    sd = env.state_dict()
    want = [env.step(a) for _ in range(15)] + [env.reset(torch.tensor([True, False, True]))]
    other = SynthTensorBlob(N, seed=9, frames="uint8")
    other.load_state_dict(sd)
    got = [other.step(a) for _ in range(15)] + [other.reset(torch.tensor([True, False, True]))]
    for w, g in zip(want[:-1], got[:-1]):
        assert all(torch.equal(x, y) for x, y in zip(w, g))
    assert torch.equal(want[-1], got[-1])
    assert all(not v.is_cuda for v in sd.values())
