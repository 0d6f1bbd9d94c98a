"""The update noise of the device generator (strict_rng=False, the mode every training run and bench.py use), GPU half: the
eps_new, eps_2, z5, z6 the kernels draw (fill_noise_rows / normal4 of csrc/dsact_kernels.h, Philox streams 1 .. 3 + fp32
Box-Muller) against tests/noise_reference.py, the NumPy restatement of include/dsact.h checked on its own in
tests/test_update_noise_host.py.

  a. k_prologue's draw (load_batch / compute_grads) == the restatement within UPDATE_NOISE_GATE, for one to five calls per row,
     batches below a block and beyond one pass of the workgroup, iterations on both sides of 2^32;
  b. the same (seed, iteration) gives the same bits on another engine, on the same engine again, through step as through
     compute_grads; apply_update (prologue without a fill) leaves the buffers alone;
  c. the gather sites (k_gather eager, the plain graph's loss rider, k_gather2 and the lookahead-2 riders of the pipelined graph).
     Which update do the debug names show after graph_build(n) + graph_run(first, n)? select_set (csrc/dsact_api.hip) copies one
     batch set's pointers over the handle's, and debug_read reads the handle's; every capture ends on select_set(h, 0). The plain
     merged graph runs update s on set (n - 1 - s) & 1 (capture_updates), the pipelined one on pipe_set((s - (n - 1)) & 3)
     (plan_updates_pipe / enqueue_updates_pipe), the CNN / unmerged graph has the one set: in all three the LAST update, s = n - 1,
     runs on set 0, and nothing stages into set 0 after it (a rider only gathers for s + 1 < n resp. s + 2 < n). So the names show
     the noise of iteration first + n - 1, a fixed function of (first, n); an eager time_steps(first, n) likewise;
  d. the CNN gathers: k_gather_img (float ring, kThreads threads per row) and k_gather_img_coded (coded ring, 64 lanes per row),
     eager and replayed;
  e. the plugin surface: DSAC_V2_HIP / DSAC_V1_HIP without strict_rng key the generator with default_noise_seed(seed).

Every comparison also requires finite values and exact zeros only where the restated radius uniform is 1.0.
"""
import numpy as np
import pytest
import torch

from helpers import hip_kwargs, synth_batch
from noise_reference import default_noise_seed, update_noise, zero_mask
from test_hip_parity import make_pair

pytestmark = pytest.mark.gpu

# max |kernel normal - restatement| over the 98 392 draws of test_prologue_draw_equals_the_restatement, measured on an MI355X
# (the gather sites, the CNN gathers and the plugin runs below stayed under it, at 1.24e-6). The
# restatement forms the uniform in float32 exactly as the kernel does, so what is left is the fp32 rounding of 2 pi u, log,
# sqrt, sin / cos and the product (the same map in NumPy float32 lies 1.6e-6 from it over 4 M draws). The gate is 4x the
# measurement.
MEASURED_UPDATE_NOISE_DIFF = 1.412e-6
UPDATE_NOISE_GATE = 4.0 * MEASURED_UPDATE_NOISE_DIFF

SEED = 0x5DEECE66D1234567      # both key words non-zero
NAMES = ("eps_new", "eps_2", "z5", "z6")
BASELINE = (376, 17, (256, 256, 256), 256)
SMALL = (16, 4, (64, 64), 64)


def read_noise(e):
    """the four noise buffers of the handle's current batch set, float32 copies shaped [B, A] / [B]"""
    B, A = e.batch, e.act_dim
    return {n: np.array(e.debug_read(n), dtype=np.float32).reshape((B, A) if n.startswith("eps") else (B,)) for n in NAMES}


def assert_noise(got, seed, it, where=""):
    """got (read_noise) == update_noise(seed, it) within the gate; finite; exact zeros only at a restated u0 of 1.0.
    Returns the largest distance."""
    B, A = got["eps_new"].shape
    worst = 0.0
    for n, want, zero in zip(NAMES, update_noise(seed, it, B, A), zero_mask(seed, it, B, A)):
        x = got[n].astype(np.float64)
        assert np.isfinite(x).all(), (where, n, it)
        d = float(np.abs(x - want).max())
        print("update noise %s it=%d B=%d A=%d %s: max |kernel - restatement| = %.3e" % (where, it, B, A, n, d))
        assert d <= UPDATE_NOISE_GATE, (where, n, it, d)
        assert np.array_equal(x == 0.0, zero), (where, n, it)
        worst = max(worst, d)
    return worst


def read_device_noise(e, seed, it):
    """the parity files' hook: the buffers of the update just computed, held to the restatement, as float32 arrays"""
    got = read_noise(e)
    assert_noise(got, seed, it, "run_case")
    return got


def share_within_gate(got, seed, it):
    """share of the elements of `got` that lie within the gate of the restatement at ANOTHER iteration"""
    B, A = got["eps_new"].shape
    hit = n = 0
    for name, want in zip(NAMES, update_noise(seed, it, B, A)):
        hit += int((np.abs(got[name] - want) <= UPDATE_NOISE_GATE).sum())
        n += want.size
    return hit / n


def _staged(O, A, hid, B, seed=SEED, **over):
    alg, _ = make_pair(O, A, hid, B, **over)
    e = alg.engine
    e.set_device_rng(seed)
    data = synth_batch(np.random.default_rng(0), B, O, A)
    e.load_batch(*(data[k].numpy() for k in ("obs", "act", "rew", "obs2", "done")))
    return alg, e


def _same_bits(a, b):
    return all(np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) for n in NAMES)


# ---- a -------------------------------------------------------------------------------------------------------------------------
_worst = {}


@pytest.mark.parametrize("O,A,hid,B,its,seeds", [
    (5, 1, (33,), 7, (0, 3), (SEED,)),                                  # a quarter of a call used; B below one 4-row block
    (11, 3, (96, 40), 50, (0, 3), (SEED,)),
    SMALL + ((0, 1, 2 ** 32 - 1, 2 ** 32 + 3, 2 ** 40 + 7), (SEED, default_noise_seed(0))),
    (23, 5, (64, 96, 64), 64, (0, 3), (SEED,)),                         # two calls per row, the second a quarter used
    BASELINE + ((0, 3), (SEED,)),                                       # five calls per row, the last a quarter used
    (8, 17, (32,), 1024, (0, 3), (SEED,)),                              # 5120 calls: twenty passes of the workgroup's loop
])
def test_prologue_draw_equals_the_restatement(O, A, hid, B, its, seeds):
    alg, e = _staged(O, A, hid, B)
    worst = 0.0
    for seed in seeds:
        e.set_device_rng(seed)
        for it in (its if seed == SEED else its[:1]):
            e.compute_grads(it)
            e.sync()
            got = read_noise(e)
            worst = max(worst, assert_noise(got, seed, it, "prologue"))
            assert not np.array_equal(got["eps_new"], got["eps_2"]) and not np.array_equal(got["z5"], got["z6"])
            e.compute_grads(it + 1)
            e.sync()
            nxt = read_noise(e)
            n = sum(got[k].size for k in NAMES)
            assert sum(int((got[k] != nxt[k]).sum()) for k in NAMES) > 0.99 * n, it
            assert share_within_gate(got, seed, it + 1) < 0.01
    _worst[(O, A, B)] = worst
    print("update noise: largest distance so far %.3e over %s" % (max(_worst.values()), sorted(_worst)))


# ---- b -------------------------------------------------------------------------------------------------------------------------
def test_seed_and_iteration_fix_the_bits():
    (_, e1), (_, e2) = _staged(*SMALL), _staged(*SMALL)
    e1.compute_grads(3); e1.sync()
    a = read_noise(e1)
    e2.compute_grads(3); e2.sync()
    assert _same_bits(a, read_noise(e2))                       # another engine
    e1.compute_grads(5); e1.sync()
    assert not _same_bits(a, read_noise(e1))
    e1.compute_grads(3); e1.sync()
    assert _same_bits(a, read_noise(e1))                       # the same engine asked again
    e1.apply_update(7); e1.sync()                              # the prologue without a fill
    assert _same_bits(a, read_noise(e1))
    e1.step(9); e1.sync()
    b = read_noise(e1)
    assert_noise(b, SEED, 9, "step")
    e2.step(9); e2.sync()
    assert _same_bits(b, read_noise(e2))                       # step draws what compute_grads draws ...
    e2.compute_grads(9); e2.sync()
    assert _same_bits(b, read_noise(e2))
    e1.step(3); e1.sync()
    assert _same_bits(a, read_noise(e1))                       # ... whatever the parameters have become


# ---- c -------------------------------------------------------------------------------------------------------------------------
def _ring(O, A, hid, B, N=2048):
    """make_pair + a filled ring and an index table, as _replay_pair of test_hip_parity.py, keyed with SEED"""
    alg, _ = make_pair(O, A, hid, B, seed=4)
    e = alg.engine
    e.set_device_rng(SEED)
    e.buffer_create(N)
    g = torch.Generator(device="cuda").manual_seed(7)
    e.buffer_fill_device(0, torch.randn(N, O, device="cuda", generator=g), torch.rand(N, A, device="cuda", generator=g) - .5,
                         torch.randn(N, device="cuda", generator=g), torch.randn(N, O, device="cuda", generator=g),
                         (torch.rand(N, device="cuda", generator=g) < .05).float())
    np.random.seed(3)
    e.upload_index_table(np.random.randint(0, N, size=(8, B)))
    return alg, e


def _assert_last_update(e, first, n, where):
    """after n updates from `first` the debug names hold the noise of iteration first + n - 1 (module docstring, c)"""
    e.sync()
    got = read_noise(e)
    last = first + n - 1
    assert_noise(got, SEED, last, where)
    for other in (last - 1, last + 1):
        assert share_within_gate(got, SEED, other) < 0.01, (where, other)


@pytest.mark.parametrize("shape,n,first,pipe", [
    (SMALL, 2, 1, None),
    (SMALL, 5, 2 ** 32 - 3, None),          # the riders' it_next + lookahead crosses 2^32 inside the replay
    (BASELINE, 2, 0, None),
    (BASELINE, 5, 6, 1.0),                  # the pipelined graph: k_gather2 and the lookahead-2 riders draw
    ((11, 3, (96, 40), 50), 3, 4, 0.0),     # tile path: the plain graph's lookahead-1 rider, a partial last gather block
])
def test_gather_sites_draw_the_restatement(shape, n, first, pipe):
    alg, e = _ring(*shape)
    assert e.time_steps(first + 11, 3, use_graph=False) > 0            # eager: k_gather per update
    _assert_last_update(e, first + 11, 3, "eager gather")
    e.graph_build(n)
    if pipe is not None:
        assert e.debug_get("pipe_graph") == pipe
    e.graph_run(first, n)
    _assert_last_update(e, first, n, "graph n=%d pipe=%d" % (n, e.debug_get("pipe_graph")))
    e.graph_run(first + n, n)                                             # a second replay continues the count
    _assert_last_update(e, first + n, n, "graph, second replay")


# ---- d -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coded", [False, True])
@pytest.mark.parametrize("A", [3, 6])
def test_cnn_gather_sites_draw_the_restatement(coded, A):
    from test_coded_image_ring import _alg_and_buffer, _samples

    B, N, shape = 16, 48, (3, 96, 96)
    alg, buf = _alg_and_buffer(coded, shape, A=A, B=B, cap=N, seed=3)
    e = alg.engine
    buf.add_batch(_samples(np.random.default_rng(7), N, shape, A))
    e.set_device_rng(SEED)
    np.random.seed(11)
    e.upload_index_table(np.random.randint(0, N, size=(4, B)))
    where = "cnn %s ring A=%d" % ("coded" if coded else "float", A)
    assert e.time_steps(2, 2, use_graph=False) > 0
    _assert_last_update(e, 2, 2, where + " eager")
    e.graph_build(2)
    e.graph_run(2 ** 32 - 1, 2)
    _assert_last_update(e, 2 ** 32 - 1, 2, where + " graph")
    buf.check()


# ---- e -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,O,A", [("DSAC_V2_HIP", 16, 4), ("DSAC_V1_HIP", 11, 3)])
def test_plugin_keys_the_generator_with_the_default_noise_seed(algo, O, A, monkeypatch):
    from dsact.engine import DsactEngine
    if algo == "DSAC_V2_HIP":
        from dsac_v2_hip import DSAC_V2_HIP as Alg
        extra = {}
    else:
        from dsac_v1_hip import DSAC_V1_HIP as Alg
        extra = {"algorithm": "DSAC_V1_HIP", "TD_bound": 10.0}
    keys = []
    plain = DsactEngine.set_device_rng

    def spy(self, seed):
        keys.append(int(seed))
        return plain(self, seed)

    monkeypatch.setattr(DsactEngine, "set_device_rng", spy)
    hid, B = (64, 64), 64
    batches = [synth_batch(np.random.default_rng(20 + it), B, O, A) for it in range(2)]
    runs = []
    for s in (1, 2, 1):
        torch.manual_seed(11)
        kw = hip_kwargs(O, A, hid, B, seed=s, **extra)
        assert "strict_rng" not in kw
        alg = Alg(**kw)
        e = alg.engine
        assert keys[-1] == default_noise_seed(s)
        drawn = []
        for it in range(2):
            alg.local_update(batches[it], it)
            e.sync()
            drawn.append(read_noise(e))
            assert_noise(drawn[-1], default_noise_seed(s), it, "%s seed=%d" % (algo, s))
        runs.append((drawn, e.online.clone()))
    assert keys == [default_noise_seed(s) for s in (1, 2, 1)]
    for it in range(2):
        assert not _same_bits(runs[0][0][it], runs[1][0][it])            # seeds 1 and 2
        assert share_within_gate(runs[1][0][it], default_noise_seed(1), it) < 0.01
        assert _same_bits(runs[0][0][it], runs[2][0][it])                # seed 1 twice
    assert torch.equal(runs[0][1], runs[2][1]) and not torch.equal(runs[0][1], runs[1][1])
