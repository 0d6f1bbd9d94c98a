"""Device-side replay index draw (opt-in: `hip_device_indices=True`, dsact_set_index_rng) -- the host side, without a GPU.

The draw is a pure function of (index seed, iteration, position, ring size) that include/dsact.h describes in words. This
file RESTATES it with Python integers from that description (nothing is imported from the library) and checks the restatement
itself: Philox4x32-10 against the published Random123 known-answer vectors, range and uniformity of the 64-bit multiply-high
map, independence from the grouping. tests/test_device_indices_gpu.py then holds the kernel to this restatement bit for bit.
Plus the host logic of HipReplayBuffer in that mode (no NumPy draw, loud refusals before any engine call, the default path
unchanged) and the exported symbols.
"""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "dsac-v2_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

M32 = 0xFFFFFFFF
INDEX_STREAM = 4          # include/dsact.h: the index draw's Philox stream id (the noise uses 1 .. 3)
SEED = 0x5DEECE66D1234567  # the seed every check below uses


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter and result
    are four 32-bit words, the key two"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw_row(seed, iteration, batch, size):
    """the `batch` indices of one iteration: counter (position / 2, iteration low, iteration high, stream 4), key = the seed's
    (low, high) word; words w[0..3] of a call are two 64-bit draws u_k = (w[2k+1] << 32) | w[2k] for positions 2p + k, and
    index = floor(u * size / 2^64)"""
    it = iteration & 0xFFFFFFFFFFFFFFFF
    out = []
    for p in range((batch + 1) // 2):
        w = philox4x32_10((p, it & M32, it >> 32, INDEX_STREAM), (seed & M32, (seed >> 32) & M32))
        for k in range(2):
            if 2 * p + k < batch:
                out.append(((w[2 * k + 1] << 32 | w[2 * k]) * size) >> 64)
    return out


def draw(seed, first_iteration, n, batch, size):
    """int64 [n][batch]: row r holds iteration first_iteration + r"""
    return np.array([draw_row(seed, first_iteration + r, batch, size) for r in range(n)], np.int64).reshape(n, batch)


# ---- 1. the generator ----------------------------------------------------------------------------------------------------------
# Random123 1.x, examples/kat_vectors, the three "philox4x32 10" lines: counter (4 words), key (2 words), expected output
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_restated_philox_matches_the_published_vectors(ctr, key, want):
    assert philox4x32_10(ctr, key) == want


# ---- 2. the map ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 2, 3, 255, 256, 257, 10_000, 10_000_019])
def test_every_index_is_in_range(size):
    rows = draw(SEED, 2 ** 32 - 3, 6, 257, size)        # odd batch (a half-used Philox call), iterations across 2^32
    assert rows.shape == (6, 257) and rows.min() >= 0 and rows.max() < size
    if size == 1:
        assert not rows.any()
    if size >= 255:
        assert len(np.unique(rows)) > 200                # (not stuck: 1542 draws hit many rows)


def test_chi_square_of_the_draw_over_256_bins():
    """2^18 draws at size 10_000 over 256 bins. 10_000 is not a multiple of 256, so the bins are the index ranges
    [floor(10_000 b / 256), floor(10_000 (b + 1) / 256)) -- 39 or 40 indices wide -- and a bin's expectation is its own width /
    10_000 of the draws. Bound: the 99.9 % quantile of chi-square with 255 degrees of freedom, 330.52
    (scipy.stats.chi2.ppf(0.999, 255); without scipy the same figure, which the Wilson-Hilferty approximation
    255 (1 - 2 / (9 * 255) + 3.0902 sqrt(2 / (9 * 255)))^3 = 330.5 confirms). The draw is deterministic: the condition holds for
    SEED or it does not (observed: 239.3)."""
    size, n_draws, bins = 10_000, 1 << 18, 256
    rows = draw(SEED, 7, n_draws // 1024, 1024, size).reshape(-1)
    edges = [(size * b) // bins for b in range(bins + 1)]
    counts = np.histogram(rows, bins=np.array(edges))[0].astype(np.float64)
    expect = n_draws * np.diff(edges) / size
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    try:
        from scipy.stats import chi2 as dist
        bound = float(dist.ppf(0.999, bins - 1))
    except ImportError:
        bound = 330.52
    print("chi-square %.2f (255 degrees of freedom; bound %.2f)" % (chi2, bound))
    assert counts.sum() == n_draws and chi2 < bound, (chi2, bound)


# ---- 3. grouping ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 5, 2 ** 32 - 4])
def test_rows_do_not_depend_on_the_grouping(first):
    one = draw(SEED, first, 8, 64, 10_000)
    for r in range(8):
        assert np.array_equal(one[r], draw(SEED, first + r, 1, 64, 10_000)[0])
    assert len({tuple(r) for r in one}) == 8             # ... and the iteration does reach the counter
    assert not np.array_equal(one, draw(SEED + 1, first, 8, 64, 10_000))
    assert not np.array_equal(one[:, :32], one[:, 32:])


# ---- 4. HipReplayBuffer -----------------------------------------------------------------------------------------------------------
class FakeEngine:
    """records the calls the buffer makes; no GPU"""

    def __init__(self, obs_dim=11, act_dim=3, batch=16, size=100):
        self.obs_dim, self.act_dim, self.batch = obs_dim, act_dim, batch
        self.buffer_size, self.buffer_ptr, self.buffer_capacity = size, size, 0
        self.rows_added = self.fill_epoch = self.stage_serial = self.index_seed = 0
        self.calls = []

    def buffer_create(self, capacity, codebook=None):
        self.buffer_capacity = capacity
        self.calls.append(("buffer_create", capacity))

    def set_index_rng(self, seed):
        self.index_seed = seed
        self.calls.append(("set_index_rng", seed))

    def draw_indices(self, it, n=1):
        self.calls.append(("draw_indices", it, n))

    def gather(self, idx):
        self.stage_serial += 1
        self.calls.append(("gather", None if idx is None else np.array(idx)))


def _kw(**over):
    return dict(dict(obsv_dim=11, action_dim=3, buffer_max_size=1000, replay_batch_size=16, seed=3), **over)


def test_device_mode_consumes_nothing_from_numpy():
    from training.hip_replay_buffer import HipReplayBuffer, index_seed_from

    e = FakeEngine()
    buf = HipReplayBuffer(**_kw(hip_engine=e, hip_device_indices=True))
    assert buf.index_seed == index_seed_from(3) and 0 < buf.index_seed < 2 ** 63
    assert e.calls == [("buffer_create", 1000), ("set_index_rng", buf.index_seed)]
    np.random.seed(5)
    before = np.random.get_state()
    grp = buf.sample_batches(16, 8)
    tok = buf.sample_batch(16)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    # the group made no engine call at all (its rows are drawn at issue); the single minibatch drew row 0 and gathered from it
    assert len(grp) == 8 and grp._idxs is None and grp._drawn == (0, 8, 100, buf.index_seed)
    assert tok._idxs is None and tok._drawn == (8, 100, buf.index_seed) and buf.index_iteration == 9
    assert [c[:3] for c in e.calls[2:]] == [("draw_indices", 8, 1), ("gather", None)]
    assert grp.device_rows(0) and grp.device_rows(3, 3) and not grp.device_rows(1)
    e.rows_added += 1                                    # a ring write: the device's rows are no longer taken blindly
    assert not grp.device_rows(0)
    # explicit seed; 0 and out-of-range values are refused
    assert HipReplayBuffer(**_kw(hip_engine=FakeEngine(), hip_device_indices=True, hip_index_seed=77)).index_seed == 77
    for bad in (0, -1, 2 ** 64):
        with pytest.raises(ValueError, match="hip_index_seed"):
            HipReplayBuffer(**_kw(hip_engine=FakeEngine(), hip_device_indices=True, hip_index_seed=bad))
    with pytest.raises(ValueError, match="empty"):
        HipReplayBuffer(**_kw(hip_engine=FakeEngine(size=0), hip_device_indices=True)).sample_batches(16, 2)


def test_mixed_modes_are_refused_before_any_engine_call(monkeypatch):
    from training import hip_replay_buffer
    from training.hip_replay_buffer import HipReplayBuffer

    class NoGpu:
        """an engine whose every call fails the test: the refusals come before anything runs"""
        obs_dim, act_dim, batch = 11, 3, 16

        def __getattr__(self, k):
            raise AssertionError("engine call %s before the refusal" % k)

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(hip_replay_buffer, "DsactEngine", no_engine)
    with pytest.raises(ValueError, match="hip_device_indices.*strict_rng"):
        HipReplayBuffer(**_kw(hip_engine=NoGpu(), hip_device_indices=True, strict_rng=True))
    monkeypatch.setattr(hip_replay_buffer, "current_engine", lambda: None)
    with pytest.raises(ValueError, match="hip_device_indices.*attached"):
        HipReplayBuffer(**_kw(hip_device_indices=True))                         # no engine to attach to
    with pytest.raises(ValueError, match="hip_device_indices.*attached"):
        HipReplayBuffer(**_kw(hip_engine=NoGpu(), hip_device_indices=True, replay_batch_size=32))   # another shape: not the algorithm's


def test_default_buffer_still_makes_the_reference_draw(monkeypatch):
    from training.hip_replay_buffer import HipReplayBuffer

    e = FakeEngine()
    buf = HipReplayBuffer(**_kw(hip_engine=e))
    assert not buf.device_indices and e.calls == [("buffer_create", 1000)]
    seen = []
    real = np.random.randint

    def spy(*a, **k):
        seen.append((a, k))
        return real(*a, **k)

    monkeypatch.setattr(np.random, "randint", spy)
    np.random.seed(9)
    grp = buf.sample_batches(16, 4)
    tok = buf.sample_batch(16)
    assert seen == [((0, 100), {"size": (4, 16)}), ((0, 100), {"size": 16})]
    np.random.seed(9)
    assert np.array_equal(grp.idxs, real(0, 100, size=(4, 16))) and np.array_equal(tok.idxs, real(0, 100, size=16))
    assert [c[0] for c in e.calls[1:]] == ["gather"] and np.array_equal(e.calls[1][1], tok.idxs)
    assert not grp.device_rows(0)


def test_rank_seeds_of_the_data_parallel_coordinator_are_distinct():
    from dsact.dp import rank_index_seed
    from training.hip_replay_buffer import index_seed_from

    assert rank_index_seed(7, 0) == index_seed_from(7)
    keys = [rank_index_seed(7, r) for r in range(64)]
    assert len(set(keys)) == 64 and all(0 < k < 2 ** 63 for k in keys)
    assert rank_index_seed(8, 1) != rank_index_seed(7, 1)


# ---- 5. the C-ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_bound():
    import ctypes as C

    from dsact import _ffi

    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    want = {
        "dsact_set_index_rng": (r"int dsact_set_index_rng\(dsact_handle\* h, uint64_t seed\);", [C.c_void_p, C.c_uint64]),
        "dsact_draw_indices": (r"int dsact_draw_indices\(dsact_handle\* h, int64_t first_iteration, int32_t n\);",
                               [C.c_void_p, C.c_int64, C.c_int32]),
        "dsact_read_indices": (r"int dsact_read_indices\(dsact_handle\* h, int64_t\* out, int32_t rows\);",
                               [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
        "dsact_run_group": (r"int dsact_run_group\(dsact_handle\* h, int64_t first_iteration, int32_t n_steps, const int64_t\* idx, "
                            r"const float\* noise, uint32_t flags\);",
                            [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.c_uint32]),
    }
    bound = {n: (res, args) for n, res, args in _ffi.SYMBOLS}
    for name, (decl, args) in want.items():
        assert re.search(decl, hdr), name
        assert bound[name] == (C.c_int, args), name
    assert "replay_buffer.py:86" in hdr[hdr.index("Device-side index draw"):hdr.index("int dsact_set_index_rng")]
    lib = _ffi.load()
    for name in want:
        assert hasattr(lib, name), name
    # without a handle the entry points refuse like every other one
    assert lib.dsact_set_index_rng(None, 1) == -1 and lib.dsact_draw_indices(None, 0, 1) == -1
    assert lib.dsact_read_indices(None, None, 1) == -1
