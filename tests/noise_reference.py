"""The update noise of the device generator (strict_rng=False: eps_new, eps_2, z5, z6 of every update) restated in NumPy from
include/dsact.h (dsact_set_device_rng) and fill_noise_rows / normal4 of csrc/dsact_kernels.h. No library call, no GPU.

  words    Philox4x32-10, counter (index, iteration low, iteration high, stream), key = the seed's (low, high) words
  index    eps_new (stream 1), eps_2 (stream 2): row * ceil(A / 4) + d // 4, element d % 4 of the call
           z5 | z6 (stream 3): index row, z5 = element 0, z6 = element 1
  uniform  u = (float32(w >> 8) + 0.5f) * 2^-24 in float32 arithmetic, as the kernel forms it: the add rounds to even once
           w >> 8 >= 2^23, so the largest value is u = 1.0 and its normal 0
  map      float64 from u on: r(u) = sqrt(-2 ln u); z0, z1 = r(u0) (cos, sin)(2 pi u1); z2, z3 = r(u2) (cos, sin)(2 pi u3)

The kernel evaluates the map in fp32; tests/test_update_noise_gpu.py holds it to this restatement within the measured distance.
"""
import numpy as np

M32 = 0xFFFFFFFF
STREAM_EPS_NEW, STREAM_EPS_2, STREAM_Z = 1, 2, 3


def default_noise_seed(seed):
    """the key DSAC_V2_HIP / DSAC_V1_HIP hand to set_device_rng when strict_rng is off (seed None counts as 0)"""
    return (int(seed or 0) * 0x9E3779B97F4A7C15 + 0x1234567) % (1 << 63) or 1


def philox_words(index, it, stream, seed):
    """uint64 [4][n]: the four 32-bit result words of Philox4x32-10 for every counter (index[i], it low, it high, stream) under
    the key (seed low, seed high); the 32-bit words travel in uint64 lanes so that the 32 x 32 products are exact"""
    it = int(it) & 0xFFFFFFFFFFFFFFFF
    m32, s32 = np.uint64(M32), np.uint64(32)
    c0 = np.asarray(index, dtype=np.uint64).reshape(-1) & m32
    c1, c2, c3 = (np.full_like(c0, v) for v in (it & M32, it >> 32, int(stream) & M32))
    k0, k1 = int(seed) & M32, (int(seed) >> 32) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack([c0, c1, c2, c3])


def eps_index(row, d, A):
    """(Philox index, element of the call) of action dimension d of minibatch row `row` in eps_new / eps_2"""
    return row * ((A + 3) // 4) + d // 4, d % 4


def uniform32(w):
    """float32: the kernel's uniform of a 32-bit word, formed in float32 arithmetic (the add rounds to even above 2^23)"""
    return (np.asarray(w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def normals(words):
    """float64 [n][4]: the Box-Muller map of the header on words [4][n]"""
    u = [uniform32(w).astype(np.float64) for w in words]
    with np.errstate(divide="ignore"):
        ra, rb = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    ta, tb = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    return np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=1)


def update_words(seed, it, B, A):
    """the words behind update_noise: (eps_new [4][B * ceil(A/4)], eps_2 likewise, z [4][B])"""
    per_row = (A + 3) // 4
    row, quad = np.repeat(np.arange(B, dtype=np.uint64), per_row), np.tile(np.arange(per_row, dtype=np.uint64), B)
    index = row * np.uint64(per_row) + quad
    return (philox_words(index, it, STREAM_EPS_NEW, seed), philox_words(index, it, STREAM_EPS_2, seed),
            philox_words(np.arange(B, dtype=np.uint64), it, STREAM_Z, seed))


def update_noise(seed, it, B, A):
    """float64 eps_new [B, A], eps_2 [B, A], z5 [B], z6 [B]: the noise of update `it` under the key `seed`"""
    per_row = (A + 3) // 4
    w_new, w_2, w_z = update_words(seed, it, B, A)
    rows = lambda w: np.ascontiguousarray(normals(w).reshape(B, per_row * 4)[:, :A])
    z = normals(w_z)
    return rows(w_new), rows(w_2), np.ascontiguousarray(z[:, 0]), np.ascontiguousarray(z[:, 1])


def zero_mask(seed, it, B, A):
    """bool eps_new [B, A], eps_2 [B, A], z5 [B], z6 [B]: the elements whose radius uniform is 1.0 in float32, i.e. whose
    normal is exactly 0 (u0 for elements 0 and 1 of a call, u2 for elements 2 and 3)"""
    per_row = (A + 3) // 4

    def one(w):
        a, b = uniform32(w[0]) == np.float32(1.0), uniform32(w[2]) == np.float32(1.0)
        return np.stack([a, a, b, b], axis=1)

    w_new, w_2, w_z = update_words(seed, it, B, A)
    rows = lambda w: one(w).reshape(B, per_row * 4)[:, :A]
    z = one(w_z)
    return rows(w_new), rows(w_2), z[:, 0], z[:, 1]
