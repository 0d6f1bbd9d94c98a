"""The reference's image pipeline on tensor environments, on the GPU (k_frame_pipe_step / k_frame_pipe_reset,
dsact_frame_pipe_step / dsact_frame_pipe_reset, training/hip_tensor_frame_pipe.py). Everything is compared
BITWISE, gray included: the fused route is one launch per inner step that computes what the torch route's ops compute -- both
are this project's rule -- and tests/test_frame_pipe_host.py holds the torch route to the reference's recording.

  1. the kernels against the torch route on the same GPU tensors: every row form, 5x7 frames (the element-wise path, one wave
     per row), 8x12 (the 16-byte path), 84x84 / 83x83 (rows split over workgroups, both paths), rows ending at every inner
     index, 14 outer steps with resets in between, every wrapper-owned output after every call, the launch counter;
  2. the C-ABI's refusals are error returns that launch nothing and leave the handle usable;
  3. inside HipTensorEnvSampler with hip_cnn_act=True: RGB bytes -> gray stack -> type_1, and codes -> a coded ring;
  4. hip_graph_sample / hip_graph_eval: replayed == eager, one case composed with wrap_tensor_env(max_episode_steps=...);
  5. eval_save on a wrapped environment records the stacks;
  6. run_state() / load_run_state() of a sampler on a wrapped environment, cut with a half-filled stack.
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

HID = (64, 64)
VEC, VEC_K = 17, 2                 # the MLP cases: [N, 17] rows stacked twice -> 34
_cache = {}


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(x, y, what):
    assert len(x) == len(y), what
    for k, (u, v) in enumerate(zip(x, y)):
        assert u.dtype == v.dtype and tuple(u.shape) == tuple(v.shape) and np.array_equal(_bits(u), _bits(v)), (what, k)


def _quiet(e):
    assert e.debug_get("act_dev_syncs") == 0.0 and e.debug_get("handoff_failures") == 0.0


@pytest.fixture(scope="module")
def shared():
    """one MLP engine (34 -> 3) for the cases that never write its weights"""
    alg, _ = make_pair(VEC * VEC_K, 3, HID, 64, seed=4)
    return alg


def _actions(N, steps, A=3):
    return [torch.from_numpy((((7 * np.arange(N)[:, None] + 3 * s + 5 * np.arange(A)[None, :]) % 9 - 4) * 0.1).astype(np.float32)).cuda()
            for s in range(steps)]


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
def _forms(h, w):
    return [("chw-u8", (3, h, w), "uint8", "chw"), ("hwc-u8", (h, w, 3), "uint8", "hwc"), ("chw-f32", (3, h, w), "float32", "chw"),
            ("hwc-f32", (h, w, 3), "float32", "hwc"), ("codes", (1, h, w), "uint8", None), ("frames-f32", (2, h, w), "float32", None),
            ("vector", (h + 1,), "float32", None), ("vector-16", (w,), "float32", None)]


def _drive(eng, N, shape, dtype, gray, K, R, fused, steps=14, limit=7):
    """reset(), then `steps` x (step, reset(ended)): every wrapper-owned output after every call as ONE byte tensor per call,
    with the survival properties and the launch counter checked on the way"""
    from synth_tensor_rgb import SynthTensorRows
    from training.hip_tensor_frame_pipe import frame_pipe_tensor_env

    env = frame_pipe_tensor_env(SynthTensorRows(N, shape, dtype, device="cuda", limit=limit), gray=gray, frame_stack=K, action_repeat=R)
    if fused:
        env.bind_engine(eng)
    else:
        env.use_fused = False
    assert env.fused == fused
    acts = _actions(N, steps)

    def flat(ts):
        return torch.cat([t.contiguous().view(torch.uint8).reshape(-1) for t in ts])

    out, ended_seen = [], []
    torch.cuda.synchronize()
    with torch.cuda.stream(eng.torch_stream):
        calls = eng.debug_get("frame_pipe_calls")
        obs = env.reset()
        calls += 1 if fused else 0
        assert eng.debug_get("frame_pipe_calls") == calls
        out.append(flat([obs, env.stack]))
        for s in range(steps):
            kept = obs.clone()
            res = env.step(acts[s])
            calls += R if fused else 0
            assert eng.debug_get("frame_pipe_calls") == calls
            assert res[0].data_ptr() != obs.data_ptr()
            out.append(flat(list(res) + [env.stack, env.ended_at, obs, kept]))          # (obs == kept: reset's return survived the step)
            ended_seen.append(env.ended_at.clone())
            kept2 = res[0].clone()
            obs = env.reset(res[2] | res[3])
            calls += 1 if fused else 0
            assert eng.debug_get("frame_pipe_calls") == calls
            out.append(flat([obs, env.stack, res[0], kept2]))                           # (res[0] == kept2: obs2 survived the reset)
        eng.sync()
    return env, out, torch.stack(ended_seen).cpu()


def _survived(rec, n_bytes):
    """the last two pieces of a record (a tensor and its earlier clone, n_bytes each) are equal"""
    return torch.equal(rec[-2 * n_bytes:-n_bytes], rec[-n_bytes:])


def _compare(eng, N, shape, dtype, gray, K, R, name):
    env_t, want, ended = _drive(eng, N, shape, dtype, gray, K, R, False)
    env_f, got, ended_f = _drive(eng, N, shape, dtype, gray, K, R, True)
    row_bytes = N * int(np.prod(env_t.obs_shape)) * env_t.stack.element_size()
    assert env_f.obs_shape == env_t.obs_shape and env_f.stack.dtype == env_t.stack.dtype
    for s, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), (name, N, K, R, s)
        if s > 0:
            assert _survived(x, row_bytes) and _survived(y, row_bytes), (name, N, K, R, s)
    assert torch.equal(ended, ended_f)
    return ended


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("N", [1, 5, 70])
def test_kernels_equal_the_torch_route(shared, N, K, R):
    eng = shared.engine
    for h, w in ((5, 7), (8, 12)):                                   # 35 elements: element-wise; 96: 16-byte accesses
        for name, shape, dtype, gray in _forms(h, w):
            ended = _compare(eng, N, shape, dtype, gray, K, R, name)
            if N >= 5:                                               # rows ended at every inner index and not at all
                assert set(ended.reshape(-1).tolist()) == set(range(-1, R)), (name, N, K, R)
    _quiet(eng)


@pytest.mark.parametrize("name,shape,dtype,gray,N,K,R", [
    ("chw-u8-84", (3, 84, 84), "uint8", "chw", 5, 4, 3),             # 1764 units of 4 pixels: 7 workgroups per row
    ("frames-f32-84", (2, 84, 84), "float32", None, 3, 2, 2),        # 3528 16-byte units: 14 workgroups per row
    ("hwc-u8-83", (83, 83, 3), "uint8", "hwc", 3, 2, 2),             # 6889 pixels, no multiple of 4: element-wise, 16 workgroups
    ("hwc-f32-84", (84, 84, 3), "float32", "hwc", 2, 1, 3),
])
def test_rows_split_over_workgroups(shared, name, shape, dtype, gray, N, K, R):
    _compare(shared.engine, N, shape, dtype, gray, K, R, name)
    _quiet(shared.engine)


def test_unaligned_rows_take_the_element_path(shared):
    """the same 8x12 frames one element into their storage: 16-byte accesses are not possible, the results are the same"""
    from training.hip_tensor_frame_pipe import frame_pipe_tensor_env

    eng = shared.engine
    N, K, R = 5, 4, 2

    class Script:
        """an 'environment' that hands out the tensors it was given"""
        num_envs = N

        def __init__(self, raws, rew, term):
            self.raws, self.rew, self.term, self.i = raws, rew, term, 0

        def reset(self, mask=None):
            return self.raws[0]

        def step(self, action):
            self.i += 1
            return self.raws[self.i % len(self.raws)], self.rew, self.term[self.i % len(self.term)], torch.zeros_like(self.term[0])

    for dtype, gray, shape in ((torch.uint8, "chw", (3, 8, 12)), (torch.float32, "hwc", (8, 12, 3)), (torch.float32, None, (2, 8, 12)),
                               (torch.uint8, None, (1, 8, 12))):
        numel = N * int(np.prod(shape))
        runs = {}
        for offset in (0, 1):
            g = torch.Generator().manual_seed(5)                     # (the same rewards and flags at either offset)
            raws = []
            for k in range(3):
                store = torch.zeros(numel + 16, dtype=dtype, device="cuda")
                vals = torch.randint(0, 256, (numel,), generator=torch.Generator().manual_seed(k)).to(dtype).cuda()
                store[offset:offset + numel].copy_(vals)
                raws.append(store[offset:offset + numel].view((N,) + shape))
                assert raws[-1].is_contiguous() and raws[-1].data_ptr() % 16 == offset * raws[-1].element_size()
            rew = torch.rand(N, generator=g).cuda()
            term = [(torch.rand(N, generator=g) < 0.3).cuda() for _ in range(4)]
            for fused in (False, True):
                env = frame_pipe_tensor_env(Script(raws, rew, term), gray=gray, frame_stack=K, action_repeat=R)
                if fused:
                    env.bind_engine(eng)
                torch.cuda.synchronize()
                out = []
                with torch.cuda.stream(eng.torch_stream):
                    out.append(env.reset().clone())
                    for s in range(4):
                        res = env.step(None)
                        out += [t.clone() for t in res] + [env.ended_at.clone()]
                        out.append(env.reset(res[2]).clone())
                    eng.sync()
                runs[(offset, fused)] = out
        for key in ((0, True), (1, False), (1, True)):
            _same(runs[key], runs[(0, False)], (str(dtype), gray, key))
    _quiet(eng)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_launch_nothing(shared):
    eng = shared.engine
    lib, h = eng._lib, eng._h
    n, P, K, R = 4, 8, 2, 3
    f = dict(dtype=torch.float32, device="cuda")
    raw, stack, out = torch.ones(n, P, **f), torch.zeros(n, K * P, **f), torch.zeros(n, K * P, **f)
    rew, acc, rew_out = torch.ones(n, **f), torch.zeros(n, **f), torch.zeros(n, **f)
    term, trunc, term_out, trunc_out = (torch.zeros(n, dtype=torch.bool, device="cuda") for _ in range(4))
    ended_at = torch.zeros(n, dtype=torch.int32, device="cuda")
    flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    host = np.zeros((n, P), np.float32)
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    calls = eng.debug_get("frame_pipe_calls")

    def step(n_=n, P_=P, K_=K, R_=R, j=0, gray=0, esize=4, raw_=p(raw), out_=p(out), acc_=p(acc)):
        return lib.dsact_frame_pipe_step(h, n_, P_, K_, R_, j, gray, esize, raw_, p(rew), p(term), p(trunc), p(stack), acc_, p(ended_at),
                                         p(flags), out_, p(rew_out), p(term_out), p(trunc_out))

    def reset(n_=n, P_=P, K_=K, gray=0, esize=4, raw_=p(raw), out_=p(out)):
        return lib.dsact_frame_pipe_reset(h, n_, P_, K_, gray, esize, raw_, None, p(stack), out_)

    INVALID = -1
    refused = [
        step(n_=0), step(n_=-1), step(K_=0), step(R_=0), step(j=-1), step(j=R), step(P_=0), step(gray=3), step(gray=-1),
        step(esize=2), step(esize=8), step(raw_=None), step(out_=None), step(acc_=None), step(raw_=C.c_void_p(host.ctypes.data)),
        reset(n_=0), reset(K_=0), reset(P_=0), reset(gray=4), reset(esize=0), reset(raw_=None), reset(out_=None),
        reset(raw_=C.c_void_p(host.ctypes.data)),
    ]
    assert refused == [INVALID] * len(refused)
    assert eng.debug_get("frame_pipe_calls") == calls                # nothing was launched
    assert reset() == 0 and all(step(j=j) == 0 for j in range(R))    # the handle is usable: the next calls succeed
    eng.sync()
    assert eng.debug_get("frame_pipe_calls") == calls + 1 + R
    assert torch.equal(out, torch.ones(n, K * P, **f)) and torch.equal(rew_out, torch.full((n,), 3.0, **f))
    assert ended_at.tolist() == [-1] * n and not term_out.any() and not trunc_out.any()
    assert eng.debug_get("handoff_failures") == 0.0


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
IMG, IMG_A, IMG_CT = (4, 84, 84), 2, "type_1"


def _cnn(book):
    """(alg, buffer) of a (4, 84, 84) type_1 handle with the CNN acting path; book: a coded ring. Built once."""
    from test_tensor_image_gpu import BOOK, _make

    key = ("cnn", book)
    if key not in _cache:
        _cache[key] = _make(IMG, IMG_A, IMG_CT, cap=64, book=BOOK if book else None)
    return _cache[key]


def _image_sampler(alg, N, S, layout, graph=False, **over):
    import plugin
    from synth_tensor_rgb import SynthTensorRgb
    from test_tensor_image_gpu import _kw

    env = SynthTensorRgb(N, device="cuda", height=84, width=84, layout=layout, frames="uint8", act_dim=IMG_A, act_limit=1.0)
    kw = _kw(IMG, IMG_A, IMG_CT, seed=3, sample_batch_size=S, sampler_name="hip_tensor_env_sampler", hip_frame_pipe=True)
    if graph:
        kw["hip_graph_sample"] = True
    return plugin.create_sampler(**dict(kw, env=env, networks=alg.networks, **over))


def _take(smp, eng):
    batch, _ = smp.sample()
    eng.sync()
    return batch, [t.detach().cpu().clone() for t in batch.device_columns]


@pytest.mark.parametrize("case", ["gray", "codes"])
def test_sampler_fused_equals_torch_route(case):
    N, S = 5, 10
    coded = case == "codes"
    alg, buf = _cnn(coded)
    eng = alg.engine
    pipe = dict(frame_stack=4) if coded else dict(frame_gray="chw", frame_stack=4, action_repeat=2)
    R = pipe.get("action_repeat", 1)
    layout = "codes" if coded else "chw"
    fused, ref = _image_sampler(alg, N, S, layout, **pipe), _image_sampler(alg, N, S, layout, **pipe)
    ref.env.use_fused = False
    row0 = buf.size
    for call in range(3):
        calls = eng.debug_get("frame_pipe_calls")
        batch, got = _take(fused, eng)
        assert fused.env.fused and eng.debug_get("frame_pipe_calls") - calls == (R + 1) * S // N
        if coded:
            buf.add_batch(batch)                                     # the byte stacks go into the coded ring as they are
            eng.sync()
        calls = eng.debug_get("frame_pipe_calls")
        _, want = _take(ref, eng)
        assert not ref.env.fused and eng.debug_get("frame_pipe_calls") == calls
        _same(got, want, call)
        obs, act, rew, obs2 = got[:4]
        assert tuple(obs.shape) == (S,) + IMG and obs.dtype == obs2.dtype == (torch.uint8 if coded else torch.float32)
        # the stack order inside the batch: a row's next observation carries its observation's newer slots, unless it restarted
        assert np.array_equal(_bits(obs2[:, :3]), _bits(obs[:, 1:]))
        if coded:
            rows = eng.buffer_export(row0 + call * S, S)
            assert rows["obs2"].dtype == np.uint8 and np.array_equal(rows["obs2"].reshape(obs2.shape), obs2.numpy())
    _quiet(eng)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def _vec_sampler(alg, N, S, graph=False, fused=True, **over):
    import plugin
    from synth_tensor_rgb import SynthTensorRows

    env = SynthTensorRows(N, (VEC,), "float32", device="cuda")
    kw = dict(sampler_name="hip_tensor_env_sampler", env=env, networks=alg.networks, sample_batch_size=S, seed=5, hip_frame_pipe=True,
              frame_stack=VEC_K, action_repeat=3)
    if graph:
        kw["hip_graph_sample"] = True
    smp = plugin.create_sampler(**dict(kw, **over))
    if not fused:
        (smp.env.env if "hip_env_wrap" in over else smp.env).use_fused = False
    return smp


@pytest.mark.parametrize("wrap", [False, True])
def test_sampler_under_hip_graph_sample(shared, wrap):
    eng = shared.engine
    N, S = 5, 20
    over = dict(hip_env_wrap=True, max_episode_steps=3) if wrap else {}
    eager, graph, torch_route = (_vec_sampler(shared, N, S, **over), _vec_sampler(shared, N, S, graph=True, **over),
                                 _vec_sampler(shared, N, S, fused=False, **over))
    assert graph.graph_sample and graph.env.capture_safe is True
    truncated = 0
    for call in range(4):                                            # eager warm-up, capture + replay, two more replays
        want = _take(eager, eng)[1]
        _same(_take(graph, eng)[1], want, call)
        _same(_take(torch_route, eng)[1], want, call)
        truncated += int(want[5].sum())
    assert graph.graph_captures == 1 and graph.graph_replays == 3
    pipe = graph.env.env if wrap else graph.env
    assert pipe.fused and torch.equal(pipe.stack, (eager.env.env if wrap else eager.env).stack)
    assert (truncated > 0) == wrap                                   # the limit counts outer steps: it fires only when it is set
    _quiet(eng)


def test_image_sampler_under_hip_graph_sample():
    N, S = 5, 10
    alg, _ = _cnn(False)
    eng = alg.engine
    pipe = dict(frame_gray="chw", frame_stack=4, action_repeat=2)
    eager, graph = _image_sampler(alg, N, S, "chw", **pipe), _image_sampler(alg, N, S, "chw", graph=True, **pipe)
    for call in range(3):                                            # eager warm-up, capture + replay, one more replay
        _same(_take(graph, eng)[1], _take(eager, eng)[1], call)
    assert graph.graph_captures == 1 and graph.graph_replays == 2 and graph.env.fused
    _quiet(eng)


def _vec_evaluator(alg, N, E, graph=False, fused=True, **over):
    import plugin
    from synth_tensor_rgb import SynthTensorRows

    env = SynthTensorRows(N, (VEC,), "float32", device="cuda")
    kw = dict(evaluator_name="hip_tensor_env_evaluator", eval_env=env, num_eval_episode=E, networks=alg.networks, hip_eval_poll_steps=4,
              hip_frame_pipe=True, frame_stack=VEC_K, action_repeat=3, hip_env_wrap=True, max_episode_steps=3)
    if graph:
        kw["hip_graph_eval"] = True
    ev = plugin.create_evaluator(**dict(kw, **over))
    if not fused:
        ev.env.env.use_fused = False
    return ev


def test_evaluator_routes_agree_under_hip_graph_eval(shared):
    from synth_tensor_rgb import ends_at

    eng = shared.engine
    N, E = 5, 13
    runs = {}
    for name, graph, fused in (("torch", False, False), ("eager", False, True), ("graph", True, True)):
        ev = _vec_evaluator(shared, N, E, graph, fused)
        out = []
        for it in range(3):
            tar = ev.run_evaluation(it)
            out.append((np.array([tar]), ev.returns.copy(), ev.lengths.copy(), ev.steps))
        runs[name] = (ev, out)
        assert ev.env.env.fused == fused
    for name in ("eager", "graph"):
        for x, y in zip(runs[name][1], runs["torch"][1]):
            assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(_bits(x[1]), _bits(y[1])), name
            assert np.array_equal(x[2], y[2]) and x[3] == y[3], name
    ev, out = runs["graph"]
    assert ev.graph_captures == 1 and ev.graph_replays >= 2
    # lengths count OUTER steps: ceil(t_end / 3) held actions, cut at the wrapper's limit of 3
    assert out[0][2].tolist() == [min(-(-ends_at(e % N, e // N) // 3), 3) for e in range(E)]
    assert eng.debug_get("handoff_failures") == 0.0


# ---- 5 -------------------------------------------------------------------------------------------------------------------------
def test_eval_save_records_the_stacks(shared, tmp_path):
    N, E = 5, 7
    ev = _vec_evaluator(shared, N, E, eval_save=True, save_folder=str(tmp_path))
    assert ev.save_max_steps == 3                                    # the outer wrapper's limit is the default step bound
    os.makedirs(str(tmp_path / "evaluator"), exist_ok=True)
    ev.run_evaluation(0)
    assert ev.trace_dropped == 0 and len(ev.saved_files) == E
    from synth_tensor_rgb import rows_value

    for e, path in enumerate(ev.saved_files):
        ep = np.load(path, allow_pickle=True).item()
        rows = np.stack(ep["obs_list"])
        r, k = e % N, e // N
        assert rows.shape == (int(ev.lengths[e]), VEC * VEC_K) and rows.dtype == np.float32
        first = rows_value(r, k, 0, (VEC,), "float32")
        assert np.array_equal(_bits(rows[0]), _bits(np.concatenate([first, first])))          # K copies of the reset frame
        for t in range(1, rows.shape[0]):                            # then one push per held action: the frame of inner step 3 t
            assert np.array_equal(_bits(rows[t, :VEC]), _bits(rows[t - 1, VEC:]))
            assert np.array_equal(_bits(rows[t, VEC:]), _bits(rows_value(r, k, 3 * t, (VEC,), "float32")))
    _quiet(shared.engine)


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
def test_run_state_resumes_a_piped_sampler_bit_for_bit():
    import plugin
    from synth_tensor_rgb import SynthTensorRows

    N, S, K = 5, 10, 4
    kw = hip_kwargs(VEC * K, 3, HID, 64, buffer_max_size=1000, seed=5, sample_batch_size=S, strict_rng=False)
    torch.manual_seed(1)
    alg = plugin.create_alg(**kw)
    eng = alg.engine

    def make():
        env = SynthTensorRows(N, (VEC,), "float32", device="cuda")
        return plugin.create_sampler(**dict(kw, sampler_name="hip_tensor_env_sampler", env=env, networks=alg.networks, hip_frame_pipe=True,
                                            frame_stack=K, action_repeat=2))

    a = make()
    _take(a, eng)                                                    # two held actions in: rows 0's stack of four is half filled
    sd = a.run_state()
    assert sd["env"]["format"] == "dsact-tensor-frame-pipe-state/1" and tuple(sd["env"]["stack"].shape) == (N, VEC * K)
    half = sd["env"]["stack"][0].view(K, VEC)
    assert torch.equal(half[0], half[1]) and not torch.equal(half[1], half[2]) and not torch.equal(half[2], half[3])
    b = make()
    b.load_run_state(sd)
    assert torch.equal(a.env.stack, b.env.stack) and b.env.fused
    ended = 0
    for call in range(3):
        x, y = _take(a, eng)[1], _take(b, eng)[1]
        _same(x, y, call)
        ended += int(x[4].sum())
    assert ended > 0                                                 # rows restarted (K copies again) inside the resumed calls
    _quiet(eng)
