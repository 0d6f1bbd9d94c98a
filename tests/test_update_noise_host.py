"""The update noise of the device generator (strict_rng=False), CPU half: tests/noise_reference.py -- the NumPy restatement of
include/dsact.h's streams 1 .. 3 that tests/test_update_noise_gpu.py and the device_noise cases of the parity files hold the
kernels to -- checked on its own:

  a. its vectorised words == a scalar restatement built on philox4x32_10 of tests/test_device_indices_host.py (pinned to the
     published Random123 vectors) and the counter layout of the header;
  b. structure: what changes the words, what shares a call, no counter used twice across rows or streams, independence of B;
  c. the normals of a fixed (seed, shape, iterations) are standard normal and uncorrelated across buffers, iterations, rows and
     columns (conditions on fixed inputs: 4.5 sigma gates);
  d. default_noise_seed == the expression DSAC_V2_HIP / DSAC_V1_HIP hand to set_device_rng.
"""
import math
import os
import re

import numpy as np
import pytest

from noise_reference import (STREAM_EPS_2, STREAM_EPS_NEW, STREAM_Z, default_noise_seed, eps_index, normals, philox_words,
                             uniform32, update_noise, update_words, zero_mask)
from test_device_indices_host import philox4x32_10

M32 = 0xFFFFFFFF
SEED = 0x5DEECE66D1234567
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsac-v2_amd")


def scalar_words(seed, it, stream, index):
    it &= 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((index & M32, it & M32, it >> 32, stream), (seed & M32, (seed >> 32) & M32))


def scalar_normal(words, e):
    """element e of the header's map on four words, in Python floats (float64) from the float32 uniform on"""
    u = [float((np.float32(w >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)) for w in words]
    r = math.sqrt(-2.0 * math.log(u[0 if e < 2 else 2]))
    t = 2.0 * math.pi * u[1 if e < 2 else 3]
    return r * (math.cos(t) if e % 2 == 0 else math.sin(t))


# ---- a -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 3, 4, 5, 17])
def test_vectorised_words_equal_the_scalar_restatement(A):
    B, per_row = 1024, (A + 3) // 4
    for it in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7):
        w_new, w_2, w_z = update_words(SEED, it, B, A)
        eps_new, eps_2, z5, z6 = update_noise(SEED, it, B, A)
        assert w_new.shape == (4, B * per_row) and w_z.shape == (4, B) and eps_new.shape == (B, A) and z5.shape == (B,)
        for row in (0, 1, 255, 256, 1023):
            for d in sorted({0, A // 2, A - 1}):
                q, e = eps_index(row, d, A)
                assert (q, e) == (row * per_row + d // 4, d % 4)
                for stream, w, out in ((1, w_new, eps_new), (2, w_2, eps_2)):
                    want = scalar_words(SEED, it, stream, q)
                    assert tuple(int(x) for x in w[:, q]) == want, (it, row, d, stream)
                    assert out[row, d] == pytest.approx(scalar_normal(want, e), abs=1e-15), (it, row, d, stream)
            want = scalar_words(SEED, it, 3, row)
            assert tuple(int(x) for x in w_z[:, row]) == want, (it, row)
            assert z5[row] == pytest.approx(scalar_normal(want, 0), abs=1e-15)
            assert z6[row] == pytest.approx(scalar_normal(want, 1), abs=1e-15)


def test_uniform_is_formed_in_float32():
    """(float)(w >> 8) + 0.5f is exact below 2^23 and rounds to even from there on: the top value is 1.0, its normal 0"""
    w = np.array([0, 1 << 8, (1 << 31) - 1, 1 << 31, (1 << 31) + (1 << 8), M32], dtype=np.uint64)
    u = uniform32(w)
    assert u.dtype == np.float32
    assert u.tolist() == [2.0 ** -25, 1.5 * 2.0 ** -24, 0.5 - 2.0 ** -25, 0.5, 0.5 + 2.0 ** -23, 1.0]
    z = normals(np.stack([np.full(4, M32, np.uint64), w[:4], w[:4], w[:4]]))
    assert not z[:, :2].any() and z[:, 2:].all()


# ---- b -------------------------------------------------------------------------------------------------------------------------
def test_every_counter_and_key_word_changes_the_words():
    base = philox_words([5], 3, STREAM_EPS_NEW, SEED)
    changed = {
        "stream": philox_words([5], 3, STREAM_EPS_2, SEED),
        "seed low word": philox_words([5], 3, STREAM_EPS_NEW, SEED ^ 1),
        "seed high word": philox_words([5], 3, STREAM_EPS_NEW, SEED ^ (1 << 32)),
        "iteration low word": philox_words([5], 4, STREAM_EPS_NEW, SEED),
        "iteration high word": philox_words([5], 3 + 2 ** 32, STREAM_EPS_NEW, SEED),
        "quad": philox_words([6], 3, STREAM_EPS_NEW, SEED),
    }
    for name, w in changed.items():
        assert (w != base).all(), name
    A = 17
    a, b = update_noise(SEED, 3, 4, A), update_noise(SEED, 3 + 2 ** 32, 4, A)
    for x, y in zip(a, b):
        assert (x != y).all()
    e0, e1 = update_noise(SEED, 3, 4, A)[0], update_noise(SEED ^ (1 << 32), 3, 4, A)[0]
    assert (e0 != e1).all()
    assert (e0[0] != e0[1]).all() and (e0[:, :4] != e0[:, 4:8]).all()       # the row and the quad reach the index


def test_the_dimensions_of_a_quad_share_one_call():
    for A in (1, 3, 4, 5, 17):
        for row in (0, 3):
            calls = [eps_index(row, d, A) for d in range(A)]
            for q in range((A + 3) // 4):
                es = [e for i, e in calls if i == calls[4 * q][0]]
                assert es == list(range(min(4, A - 4 * q))), (A, row, q)


@pytest.mark.parametrize("A", [5, 17])
def test_a_rows_last_quad_is_not_the_next_rows_first(A):
    B = 64
    idx = np.array([[eps_index(r, d, A)[0] for d in range(A)] for r in range(B)])
    assert (idx[:-1, -1] != idx[1:, 0]).all() and (idx[:-1, -1] + 1 == idx[1:, 0]).all()
    assert len(np.unique(idx)) == B * ((A + 3) // 4)
    eps_new = update_noise(SEED, 0, B, A)[0]
    assert (eps_new[:-1, A - 1] != eps_new[1:, 0]).all()
    # the unused elements of a row's last call do not leak into the next row
    full = normals(update_words(SEED, 0, B, A)[0]).reshape(B, -1)
    assert (full[:-1, A] != eps_new[1:, 0]).all()


def test_the_three_streams_use_pairwise_distinct_counters():
    B, A = 1024, 17
    per_row = (A + 3) // 4
    sets = {
        "eps_new": {(eps_index(r, d, A)[0], STREAM_EPS_NEW) for r in range(B) for d in range(A)},
        "eps_2": {(eps_index(r, d, A)[0], STREAM_EPS_2) for r in range(B) for d in range(A)},
        "z": {(r, STREAM_Z) for r in range(B)},
    }
    assert len(sets["eps_new"]) == len(sets["eps_2"]) == B * per_row and len(sets["z"]) == B
    names = list(sets)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not (sets[a] & sets[b]), (a, b)
    w_new, w_2, w_z = update_words(SEED, 0, B, A)
    words = np.concatenate([w_new, w_2, w_z], axis=1).T
    assert len(np.unique(words, axis=0)) == 2 * B * per_row + B


def test_a_rows_noise_does_not_depend_on_the_batch_size():
    for A in (3, 17):
        big = update_noise(SEED, 9, 1024, A)
        for B in (1, 7, 256):
            for x, y in zip(update_noise(SEED, 9, B, A), big):
                assert np.array_equal(x, y[:B]), (A, B)


# ---- c -------------------------------------------------------------------------------------------------------------------------
def _corr_sigmas(x, y):
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    return float(np.corrcoef(x, y)[0, 1] * math.sqrt(x.size))


def test_the_restated_normals_are_standard_and_uncorrelated():
    seed, B, A, T = default_noise_seed(7), 256, 17, 16
    draws = [update_noise(seed, it, B, A) for it in range(T)]
    eps_new, eps_2 = np.stack([d[0] for d in draws]), np.stack([d[1] for d in draws])      # [T, B, A]
    z5, z6 = np.stack([d[2] for d in draws]), np.stack([d[3] for d in draws])              # [T, B]
    z = np.concatenate([a.reshape(-1) for a in (eps_new, eps_2, z5, z6)])
    n = z.size
    assert n == 147456
    assert np.isfinite(z).all() and np.abs(z).max() < 5.9
    p = 0.682689
    figures = {"mean": z.mean() * math.sqrt(n), "variance": (z.var() - 1.0) / math.sqrt(2.0 / n),
               "P(|z| < 1)": ((np.abs(z) < 1.0).mean() - p) / math.sqrt(p * (1.0 - p) / n)}
    corr = {"eps_new ~ eps_2": _corr_sigmas(eps_new, eps_2), "z5 ~ z6": _corr_sigmas(z5, z6),
            "iteration t ~ t + 1": _corr_sigmas(eps_new[:-1], eps_new[1:]), "row r ~ r + 1": _corr_sigmas(eps_new[:, :-1], eps_new[:, 1:]),
            "column d ~ d + 1": _corr_sigmas(eps_new[:, :, :-1], eps_new[:, :, 1:]), "eps_new[:, 0] ~ z5": _corr_sigmas(eps_new[:, :, 0], z5)}
    print({k: round(float(v), 2) for k, v in {**figures, **corr}.items()})
    for name, v in {**figures, **corr}.items():
        assert abs(v) < 4.5, (name, v)


def test_exact_zeros_are_the_top_uniform_only():
    """the mask of restated u0 == 1.0 is exactly where the restated normal is 0 (2^-25 of the draws; none at this size is fine)"""
    seed, B, A = default_noise_seed(7), 256, 17
    for it in range(4):
        for x, m in zip(update_noise(seed, it, B, A), zero_mask(seed, it, B, A)):
            assert np.array_equal(x == 0.0, m)
    w = np.stack([np.array([M32, 5 << 8], np.uint64)] * 4)
    assert np.array_equal(normals(w) == 0.0, [[True] * 4, [False] * 4])


# ---- d -------------------------------------------------------------------------------------------------------------------------
def test_default_noise_seed():
    assert default_noise_seed(0) == default_noise_seed(None) == 0x1234567 and default_noise_seed(1) != 0
    seeds = [default_noise_seed(s) for s in range(1000)]
    assert len(set(seeds)) == 1000 and all(0 < s < 1 << 63 for s in seeds)
    assert default_noise_seed(1) == (0x9E3779B97F4A7C15 + 0x1234567) % (1 << 63)


@pytest.mark.parametrize("plugin", ["dsac_v2_hip.py", "dsac_v1_hip.py"])
def test_default_noise_seed_is_the_plugins_expression(plugin):
    with open(os.path.join(PKG, plugin)) as f:
        src = f.read()
    found = re.findall(r"self\.engine\.set_device_rng\((.+)\)\s*$", src, flags=re.M)
    assert len(found) == 1, found
    for seed in (0, 1, 2, 7, 12345, 2 ** 31 - 1, 2 ** 40 + 3):
        assert eval(found[0], {"seed": seed}) == default_noise_seed(seed), (plugin, seed)
