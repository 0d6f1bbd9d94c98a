"""Device-side replay index draw on the GPU (k_draw_indices, dsact_set_index_rng / dsact_draw_indices / dsact_read_indices,
dsact_run_group with idx == NULL, HipReplayBuffer(hip_device_indices=True)).

  6. the kernel == the Python restatement of tests/test_device_indices_host.py (itself pinned to the published Philox
     vectors), bit for bit;
  7. a group whose rows the device draws == the same group given those rows from the host: only where the indices come from
     changed (parameters, targets, both Adam moments, step state, statistics, the staged minibatch);
  8. group == per-update through the plugin surface, also with DSACT_F_SKIP_ACTOR_ON_OFF_ITERS and a misaligned start;
  9. the serial and the overlapped trainer run in that mode (reduced form, see the test's docstring);
 10. a stale token re-gathers its own rows and raises once one of them was overwritten.
"""
import numpy as np
import pytest
import torch

from helpers import hip_kwargs
from oracle.trainer_trajectory import variant_case
from test_device_indices_host import SEED, draw
from test_hip_groups import _family_alg, fill, host_ring, same_engine_state

pytestmark = pytest.mark.gpu


def _engine(B, hid=(64, 64), O=16, A=4, **over):
    from test_hip_parity import make_pair

    alg, _ = make_pair(O, A, hid, B, seed=4, **over)
    return alg.engine


# ---- 6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [16, 256, 1024])
def test_kernel_equals_the_restatement(B):
    e = _engine(B)
    e.buffer_create(10_000)
    e.set_index_rng(SEED)
    with pytest.raises(Exception, match="buffer empty"):
        e.draw_indices(0, 1)                                   # np.random.randint(0, 0) raises too
    rng = np.random.default_rng(0)
    size = 0
    for want_size in (1, 257, 10_000):                         # the ring grows: the draw takes its size at issue time
        n = want_size - size
        e.buffer_add(rng.standard_normal((n, 16), dtype=np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32),
                     rng.standard_normal((n, 16), dtype=np.float32), np.zeros(n, np.float32))
        size = want_size
        assert e.buffer_size == size
        for n_rows in (1, 8, 64):
            for first in (0, 2 ** 32 - 5, 2 ** 32 + 3, 2 ** 40 + 7):
                if n_rows == 64 and first not in (0, 2 ** 32 - 5):
                    continue                                   # (64 rows: once at 0 and once across 2^32)
                e.draw_indices(first, n_rows)
                got = e.read_indices(n_rows)
                assert got.dtype == np.int64 and got.shape == (n_rows, B)
                assert np.array_equal(got, draw(SEED, first, n_rows, B, size)), (B, size, n_rows, first)
    # the seed reaches the key, both words of it
    e.draw_indices(3, 2)
    a = e.read_indices(2)
    for seed in (SEED ^ 1, SEED ^ (1 << 40)):
        e.set_index_rng(seed)
        e.draw_indices(3, 2)
        b = e.read_indices(2)
        assert np.array_equal(b, draw(seed, 3, 2, B, size)) and not np.array_equal(a, b)
    # the drawn row is what dsact_gather(NULL) stages
    e.set_index_rng(SEED)
    e.draw_indices(11, 1)
    e.gather(None)
    row = e.read_indices(1)[0]
    staged = e.read_batch()
    e.gather(row)
    again = e.read_batch()
    for k in staged:
        assert np.array_equal(staged[k], again[k]), k
    # switched off: NULL rows are refused, and the message says what to call
    e.set_index_rng(0)
    e.set_device_rng(5)
    with pytest.raises(Exception, match="dsact_set_index_rng"):
        e.run_group(0, None, n=2)
    with pytest.raises(Exception, match="dsact_set_index_rng"):
        e.draw_indices(0, 1)


def test_odd_batch_rows_keep_their_neighbours():
    """a ragged batch: the last Philox call of a row is half used, and row r + 1 starts at an odd element offset"""
    B = 50
    e = _engine(B, hid=(96, 40), O=11, A=3)
    fill(e, host_ring(777, 11, 3, 1))
    e.set_index_rng(SEED)
    e.draw_indices(9, 16)
    assert np.array_equal(e.read_indices(16), draw(SEED, 9, 16, B, 777))


# ---- 7 -------------------------------------------------------------------------------------------------------------------------
def _mlp_engines(O, A, hid, B, algo="v2", **over):
    out = []
    for _ in range(2):
        if algo == "v1":
            e = _family_alg("v1_mlp", B, seed=4)[0].engine
        else:
            e = _engine(B, hid, O, A, **over)
        out.append(e)
    return out


@pytest.mark.parametrize("name,O,A,hid,B,first,lengths", [
    ("baseline_pipelined", 376, 17, (256, 256, 256), 256, 3, [8, 8, 5]),
    ("batch_1024", 376, 17, (256, 256, 256), 1024, 0, [4, 4]),
    ("ragged_tiles", 11, 3, (96, 40), 50, 1, [4, 5]),
    ("v1", 16, 4, (64, 64), 64, 1, [8, 3, 8]),
])
def test_device_rows_equal_the_same_rows_from_the_host(name, O, A, hid, B, first, lengths):
    N = 3000
    ring = host_ring(N, O, A, 3)
    dev, host = _mlp_engines(O, A, hid, B, algo="v1" if name == "v1" else "v2")
    for e in (dev, host):
        e.set_device_rng(4242)
        fill(e, ring)
        e.set_index_rng(SEED)
    it = first
    for n in lengths:
        dev.run_group(it, None, n=n)
        host.draw_indices(it, n)
        rows = host.read_indices(n)
        assert np.array_equal(rows, draw(SEED, it, n, B, N))
        host.run_group(it, rows)
        it += n
    dev.sync()
    host.sync()
    same_engine_state(dev, host, name)
    assert np.array_equal(dev.read_indices(lengths[-1]), host.read_indices(lengths[-1]))
    assert torch.isfinite(dev.online).all()
    assert dev.debug_get("pipe_graph") == host.debug_get("pipe_graph") and dev.debug_get("graph_cache") == host.debug_get("graph_cache")
    if name == "baseline_pipelined":
        assert dev.chain_active and dev.debug_get("pipe_graph") == 1.0


@pytest.mark.parametrize("coded", [False, True])
def test_device_rows_equal_host_rows_cnn(coded):
    from test_coded_image_ring import BOOK

    B, N, first, lengths = 16, 64, 3, [5, 8]
    O, A = 3 * 96 * 96, 3
    engines = []
    for _ in range(2):
        e = _family_alg("v2_cnn", B, seed=4)[0].engine
        e.set_device_rng(4242)
        e.buffer_create(N, codebook=BOOK if coded else None)
        g = torch.Generator(device="cuda").manual_seed(9)
        book = torch.as_tensor(BOOK, device="cuda")
        e.buffer_fill_device(0, book[torch.randint(0, 256, (N, O), device="cuda", generator=g)].contiguous(),
                             torch.rand(N, A, device="cuda", generator=g) * 0.8 - 0.4, torch.randn(N, device="cuda", generator=g),
                             book[torch.randint(0, 256, (N, O), device="cuda", generator=g)].contiguous(),
                             (torch.rand(N, device="cuda", generator=g) < .1).float())
        e.set_index_rng(SEED)
        engines.append(e)
    dev, host = engines
    it = first
    for n in lengths:
        dev.run_group(it, None, n=n)
        host.draw_indices(it, n)
        host.run_group(it, host.read_indices(n))
        it += n
    dev.sync()
    host.sync()
    host.buffer_check()
    same_engine_state(dev, host, "cnn coded=%s" % coded)
    assert torch.isfinite(dev.online).all()


# ---- 8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,first", [(0, 0), (0, 5), (1, 0), (1, 3)])
def test_group_equals_per_update_through_the_plugin_surface(flags, first):
    """n = 8 through sample_batches + local_update_group == 8 x { sample_batch; local_update }; with
    DSACT_F_SKIP_ACTOR_ON_OFF_ITERS and a misaligned start the group is issued as head updates + an aligned replay + tail
    updates, and the pieces draw by iteration"""
    from dsac_v2_hip import DSAC_V2_HIP
    from training.hip_replay_buffer import HipReplayBuffer

    O, A, hid, B, N, K = 16, 4, (64, 64), 64, 500, 8
    ring = host_ring(N, O, A, 9)
    out = []
    for mode in ("single", "group"):
        torch.manual_seed(2)
        kw = hip_kwargs(O, A, hid, B, buffer_max_size=N, seed=5, hip_flags=flags, hip_device_indices=True)
        alg = DSAC_V2_HIP(**kw)
        buf = HipReplayBuffer(**kw)
        assert buf.engine is alg.engine and buf.device_indices and alg.engine.index_seed == buf.index_seed
        samples = [(ring["obs"][i], {}, ring["act"][i], float(ring["rew"][i]), ring["obs2"][i], bool(ring["done"][i]), 0.0, {})
                   for i in range(N)]
        buf.add_batch(samples)
        buf.index_iteration = first                      # the minibatch counter follows the caller's iteration
        np.random.seed(3)
        if mode == "group":
            grp = buf.sample_batches(B, K)
            tb = alg.local_update_group(grp, first)
            assert grp._idxs is None                     # no index ever reached the host
            tb = alg.local_update_group(buf.sample_batches(B, 3), first + K)
        else:
            for it in range(first, first + K + 3):
                tok = buf.sample_batch(B)
                tb = alg.local_update(tok, it)
                assert tok._idxs is None
        vals = [float(tb[k]) for k in sorted(tb.keys()) if "Time" not in k]
        out.append((alg, vals, np.random.randint(0, 1 << 30)))
    np.random.seed(3)
    assert out[0][2] == out[1][2] == np.random.randint(0, 1 << 30)      # the NumPy stream was never touched
    assert out[0][1] == out[1][1]
    same_engine_state(out[0][0].engine, out[1][0].engine, "flags %d first %d" % (flags, first))
    assert torch.isfinite(out[1][0].engine.online).all()


# ---- 9 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("trainer", ["serial", "async"])
def test_trainers_run_with_device_indices(tmp_path, K, trainer):
    """REDUCED form. The full form would feed a CPU oracle loop the restated indices and the same noise; the noise of a run with
    strict_rng=False is drawn inside the update kernels and cannot be injected on both sides, and strict_rng=True is refused
    together with hip_device_indices. So: everything the loop decides that does not depend on the arithmetic is compared with
    the CPU oracle loop of tests/test_async_trainer_host.py exactly (ring size / ptr at every draw, group lengths, sample
    counts, warm-up, scalar tags and steps, checkpoint names), every logged value is finite, no hand-over failed, and the last
    group's rows are the restated draw."""
    import plugin
    from test_async_trainer_host import _async, _lagged_serial_cls, _serial, derived_kwargs, run_loop

    case = dict(variant_case("si%d" % K), algorithm="DSAC_V2_HIP")
    cpu_trainer = _lagged_serial_cls() if trainer == "async" else _serial
    want, _ = run_loop(derived_kwargs(case, str(tmp_path / "cpu")), cpu_trainer)

    kw = derived_kwargs(dict(case, buffer_name="hip_replay_buffer"), str(tmp_path / "hip"), hip_device_indices=True)
    alg = plugin.create_alg(**kw)
    buffer = plugin.create_buffer(**kw)
    assert buffer.engine is alg.engine and buffer.device_indices and not alg.strict_rng
    got, tr = run_loop(kw, _async if trainer == "async" else _serial, alg=alg, buffer=buffer)
    e = alg.engine
    assert e.debug_get("handoff_failures") == 0.0
    for k in ("buffer", "saved", "apprfunc_dir", "warm", "samples"):
        assert got[k] == want[k], k
    assert got["indices"] == []                          # no np.random.randint call was made by the loop
    assert [t[:2] for t in got["tb"]] == [t[:2] for t in want["tb"]]
    assert any(t[1] >= 2 for t in got["tb"])
    assert [e_[0] for e_ in got["evals"]] == [e_[0] for e_ in want["evals"]]
    assert len(got["scalars"]) == len(want["scalars"])
    wall = "Evaluation/2. TAR-Total time [s]"
    for g, w in zip(got["scalars"], want["scalars"]):
        assert g[0] == w[0] and (g[0] == wall or g[1] == w[1]), (g, w)
        assert np.isfinite(g[2]), g
    for t in got["tb"]:
        assert np.isfinite(t[2:]).all(), t
    assert buffer.index_iteration == case["max_iteration"] == tr.iteration
    n_last = got["tb"][-1][1]
    assert np.array_equal(e.read_indices(n_last), draw(buffer.index_seed, tr.iteration - n_last, n_last, e.batch, buffer.size))
    torch.cuda.synchronize()


# ---- 10 ------------------------------------------------------------------------------------------------------------------------
def test_stale_token_regathers_its_rows_and_raises_once_overwritten():
    from dsac_v2_hip import DSAC_V2_HIP
    from training.hip_replay_buffer import HipReplayBuffer

    O, A, hid, B, N = 16, 4, (64, 64), 16, 200
    ring = host_ring(N, O, A, 9)
    ring["rew"] = np.arange(N, dtype=np.float32)          # the reward of row i is i
    torch.manual_seed(2)
    kw = hip_kwargs(O, A, hid, B, buffer_max_size=N, seed=5, hip_device_indices=True)
    alg = DSAC_V2_HIP(**kw)
    buf = HipReplayBuffer(**kw)
    e = alg.engine
    e.buffer_add(ring["obs"], ring["act"], ring["rew"], ring["obs2"], ring["done"])
    first, second = buf.sample_batch(B), buf.sample_batch(B)
    want_first, want_second = draw(buf.index_seed, 0, 1, B, N)[0], draw(buf.index_seed, 1, 1, B, N)[0]
    assert np.array_equal(e.read_batch()["rew"], want_second.astype(np.float32))      # `second` is staged; `first` is stale
    # stale, ring untouched: the same draw again on the device, no index fetched
    first.restage()
    assert first._idxs is None and np.array_equal(e.read_batch()["rew"], want_first.astype(np.float32))
    # reading a stale token as a dict: its own rows
    assert np.array_equal(second["rew"].numpy(), want_second.astype(np.float32))
    assert np.array_equal(second["obs"].numpy(), ring["obs"][want_second])
    # rows written that are none of the token's: it fetches its indices (the slow path), checks them, re-gathers them
    third = buf.sample_batch(B)
    want_third = draw(buf.index_seed, 2, 1, B, N)[0]
    assert e.buffer_ptr == 0 and e.buffer_size == N       # the ring is full: the next writes replace rows 0, 1, ...
    n_free = int(want_third.min())                        # rows [0, n_free) are none of the token's
    if n_free:
        e.buffer_add(ring["obs"][:n_free], ring["act"][:n_free], ring["rew"][:n_free], ring["obs2"][:n_free], ring["done"][:n_free])
        buf.sample_batch(B)                                                            # `third` goes stale
        alg.local_update(third, 0)
        assert np.array_equal(third.idxs, want_third)
        assert np.array_equal(e.read_batch()["rew"], want_third.astype(np.float32))
    # ... and one more row -- one of its own -- makes it refuse
    e.buffer_add(ring["obs"][:1], ring["act"][:1], -np.ones(1, np.float32), ring["obs2"][:1], ring["done"][:1])
    buf.sample_batch(B)
    with pytest.raises(RuntimeError, match="overwritten"):
        alg.local_update(third, 1)
    grp = buf.sample_batches(B, 2)
    e.buffer_add(ring["obs"], ring["act"], ring["rew"], ring["obs2"], ring["done"])    # the whole ring
    with pytest.raises(RuntimeError, match="overwritten"):
        alg.local_update_group(grp, buf.index_iteration - 2)
    e.sync()
