"""HipReplayBuffer -- device-resident replay ring; drop-in for reference training/replay_buffer.py.

Discovered by the reference's rule `create_buffer(buffer_name="hip_replay_buffer")` -> module
`training.hip_replay_buffer`, class `HipReplayBuffer` (reference utils/initialization.py:90-117).

Same observable behaviour as the reference ReplayBuffer (replay_buffer.py:20-90): SoA fp32 ring with
`ptr=(ptr+1)%N`, `size=min(size+1,N)`, uniform index draw with replacement from the GLOBAL legacy
NumPy RandomState (`np.random.randint(0, size, batch)`, bit-exact by construction because the very
same call is made here on the host), `sample_batch` returns a dict with keys
obs/obs2/act/rew/done/logp. The rows live in HBM; the gather is a HIP kernel (k_gather) that writes
straight into the update's staging area, and the returned `HipBatch` is a token for it.

`hip_obs_codebook=table` (image observations only) stores the obs / obs2 columns as one byte per element, an index into
`table` (at most 256 float32 values, strictly ascending): a quarter of the fp32 ring's bytes, bit-identical minibatches.
CarRacing's frames (`rgb / 255` cast to float32) take `np.float32(np.arange(256) / 255.0)`. See parse_obs_codebook.

`hip_device_indices=True` (opt-in) moves the index draw to the device: uniform with replacement in [0, size) like the
reference's, from Philox4x32-10 keyed by (index seed, minibatch counter, position) -- include/dsact.h, dsact_set_index_rng.
No np.random call is made, so the run is reproducible from its seeds but is NOT index for index the reference's run, exactly
as `strict_rng=False` is for the noise. The minibatch counter `index_iteration` starts at 0 and advances by one per minibatch
drawn: in the reference's loop (one minibatch per update, iterations from 0) it IS the trainer's iteration, which is what
makes a group's rows equal the per-update draws; a caller that starts elsewhere assigns it. `hip_index_seed` (default:
index_seed_from(seed)) is the Philox key; the noise of `strict_rng=False` uses other stream ids of the same generator, so the
two never share a counter block whatever the seeds.

`add_batch` also takes a `DeviceSampleBatch` (training/hip_tensor_sampler.py: the transitions of a batched tensor environment,
already on the GPU) and hands its seven device tensors to the ring in one asynchronous call (dsact_buffer_add_device); every
other input takes the paths it always took.
"""
import numpy as np

from dsact.engine import DsactEngine, current_engine

__all__ = ["HipReplayBuffer", "parse_obs_codebook", "index_seed_from", "act_seed_from"]

MAX_CODES = 256


def index_seed_from(seed):
    """default `hip_index_seed` of a run with the global `seed`: an odd-multiplier affine map into [1, 2^63) (0 would switch
    the draw off). Any value works -- independence from the noise comes from the Philox stream id, not from this map."""
    return (int(seed or 0) * 0xD1342543DE82EF95 + 0x2545F4914F6CDD1D) % (1 << 63) or 1


def act_seed_from(seed):
    """default `hip_act_seed` of a run with the global `seed` (training/hip_tensor_sampler.py: the Philox key of the in-kernel
    acting noise): another fixed odd-multiplier affine map into [1, 2^63), so that a run's index draw and acting noise do not
    share a key by default either (their Philox stream ids, 4 and 5, already keep them apart for ANY pair of seeds)."""
    return (int(seed or 0) * 0x9FB21C651E98DF25 + 0x6A09E667F3BCC909) % (1 << 63) or 1


def parse_obs_codebook(table, obs_shape):
    """Validates `hip_obs_codebook` for observations of shape `obs_shape` and returns it as a float32 array (no GPU call).
    The table is cast to float32 first and must then be strictly ascending as floats: no NaN, no duplicates, not both -0.0
    and 0.0 (a stored value matches an entry only if the bit patterns are equal). Observations must be images (C, H, W)
    with H * W % 16 == 0 and C <= 16 (the coded gather loads 16 codes of a plane per lane)."""
    shape = tuple(int(d) for d in obs_shape)
    if len(shape) != 3:
        raise NotImplementedError("hip_obs_codebook: codes are for image observations (C, H, W); obsv_dim %r is not one" % (shape,))
    C, H, W = shape
    if (H * W) % 16 or C > 16:
        raise NotImplementedError("hip_obs_codebook: a coded ring needs H * W %% 16 == 0 and C <= 16 (obsv_dim %r)" % (shape,))
    t = np.asarray(table)
    if t.ndim != 1 or t.size == 0:
        raise ValueError("hip_obs_codebook: a 1-D list of 1 .. %d values, got shape %r" % (MAX_CODES, t.shape))
    if t.size > MAX_CODES:
        raise ValueError("hip_obs_codebook: %d entries, at most %d (one byte per code)" % (t.size, MAX_CODES))
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.ascontiguousarray(t.astype(np.float32))
    if np.isnan(f).any():
        raise ValueError("hip_obs_codebook: entry %d is NaN" % int(np.flatnonzero(np.isnan(f))[0]))
    bad = np.flatnonzero(~(f[1:] > f[:-1]))
    if bad.size:
        i = int(bad[0])
        raise ValueError("hip_obs_codebook: after the float32 cast entries %d, %d are not strictly ascending (%r, %r); "
                         "duplicates and a -0.0 / 0.0 pair are refused" % (i, i + 1, float(f[i]), float(f[i + 1])))
    return f


class HipReplayBuffer:
    def __init__(self, index=0, **kwargs):
        self.obsv_dim = kwargs["obsv_dim"]   # int, or the (C, H, W) tuple of the CNN configs (replay_buffer.py:22-31)
        self._obs_shape = tuple(self.obsv_dim) if isinstance(self.obsv_dim, (tuple, list)) else (int(self.obsv_dim),)
        self._obs_flat = int(np.prod(self._obs_shape))
        self.act_dim = kwargs["action_dim"]
        self.max_size = int(kwargs["buffer_max_size"])
        if kwargs.get("additional_info"):
            raise NotImplementedError("additional_info is not supported by HipReplayBuffer")
        book = kwargs.get("hip_obs_codebook")
        self.codebook = None if book is None else parse_obs_codebook(book, self._obs_shape)
        self.device_indices = bool(kwargs.get("hip_device_indices", False))
        if self.device_indices and kwargs.get("strict_rng", False):
            raise ValueError("hip_device_indices=True with strict_rng=True: a parity run wants the reference's np.random.randint "
                             "indices as well as its torch.randn noise; drop one of the two kwargs")
        eng = kwargs.get("hip_engine") or current_engine()
        B = int(kwargs["replay_batch_size"])
        if self.device_indices and (eng is None or eng.obs_dim != self._obs_flat or eng.act_dim != self.act_dim or eng.batch != B):
            raise ValueError("hip_device_indices=True needs the buffer attached to the algorithm's engine (create the algorithm "
                             "first, or pass hip_engine=): the device draws the indices where the update reads them")
        if eng is None or eng.obs_dim != self._obs_flat or eng.act_dim != self.act_dim or eng.batch != B:
            if len(self._obs_shape) == 3:
                from dsact.layout import CONV_TYPES
                ct = kwargs.get("value_conv_type", "type_2")
                eng = DsactEngine(self._obs_shape, self.act_dim, CONV_TYPES[ct][4], B, conv_type=ct,
                                  device=int(kwargs.get("hip_device", 0)))
            else:
                hidden = list(kwargs.get("value_hidden_sizes", [32]))
                eng = DsactEngine(self._obs_flat, self.act_dim, hidden, B, device=int(kwargs.get("hip_device", 0)))
        self.engine = eng
        self.engine.buffer_create(self.max_size, codebook=self.codebook)
        self.index_seed, self.index_iteration = 0, 0
        if self.device_indices:
            seed = kwargs.get("hip_index_seed")
            self.index_seed = int(seed) if seed is not None else index_seed_from(kwargs.get("seed"))
            if not 0 < self.index_seed < (1 << 64):
                raise ValueError("hip_index_seed must be in [1, 2^64) (0 switches the device draw off), got %r" % (seed,))
            self.engine.set_index_rng(self.index_seed)

    @property
    def size(self):
        return self.engine.buffer_size

    @property
    def ptr(self):
        return self.engine.buffer_ptr

    def __len__(self):
        return self.size

    def __get_RAM__(self):
        obs_bytes = 2 * self._obs_flat * (1 if self.codebook is not None else 4)
        row_bytes = obs_bytes + 4 * (self.act_dim + 3)
        return row_bytes * self.size / 1e6  # MB resident in HBM

    def check(self):
        """synchronous: raises DsactError if an observation value missing from `hip_obs_codebook` was stored"""
        self.engine.buffer_check()

    def store(self, obs, info, act, rew, next_obs, done, logp, next_info):
        self.add_batch([(obs, info, act, rew, next_obs, done, logp, next_info)])

    def add_batch(self, samples: list):
        n = len(samples)
        if n == 0:
            return
        cols = getattr(samples, "device_columns", None)
        if cols is not None:
            # a DeviceSampleBatch (training/hip_tensor_sampler.py): the transitions are device tensors -- ONE ring commit, no copy
            if n > self.max_size:
                raise ValueError("a device batch of %d transitions does not fit a ring of %d rows" % (n, self.max_size))
            self.engine.buffer_add_device(*cols, reward_scale=samples.reward_scale)
            return
        packed = getattr(samples, "packed", None)
        if packed is not None and packed[0].shape == (n, self._obs_flat) and self._packed_matches(samples, packed):
            # HipOffSampler's fast path already holds the transitions as packed float32 arrays (training/hip_sampler.py)
            obs, act, rew, obs2, done, logp = packed
            self.engine.buffer_add(obs, act, rew, obs2, done, logp)
            return
        O, A = self._obs_flat, self.act_dim
        obs = np.empty((n, O), np.float32)
        obs2 = np.empty((n, O), np.float32)
        act = np.empty((n, A), np.float32)
        rew = np.empty(n, np.float32)
        done = np.empty(n, np.float32)
        logp = np.empty(n, np.float32)
        for i, s in enumerate(samples):
            obs[i], act[i], rew[i], done[i], logp[i] = np.asarray(s[0]).reshape(-1), s[2], s[3], s[5], s[6]
            obs2[i] = np.asarray(s[4]).reshape(-1)
        self.engine.buffer_add(obs, act, rew, obs2, done, logp)

    @staticmethod
    def _packed_matches(samples, packed):
        """the packed arrays are only trusted while the list still is what the sampler built: a consumer that filtered,
        reordered or replaced tuples (reward shaping, n-step post-processing) gets the tuple walk. Checked on the first,
        middle and last tuple: their action must still BE the packed row (same memory) and their reward the packed value."""
        n = len(samples)
        try:
            for i in {0, n // 2, n - 1}:
                t = samples[i]
                a = t[2]
                if not (isinstance(a, np.ndarray) and a.ctypes.data == packed[1][i].ctypes.data):
                    return False
                if np.float32(t[3]) != packed[2][i] or bool(t[5]) != bool(packed[4][i]):
                    return False
        except Exception:
            return False
        return True

    def sample_batches(self, batch_size: int, n: int):
        """the index rows of the next `n` minibatches: n x `np.random.randint(0, size, batch_size)` -- the calls, and the
        order, of n reference `sample_batch` calls with no add_batch between them (replay_buffer.py:86; the ring size is
        constant, nothing else consumes the NumPy stream). The rows are gathered on the device by
        DSAC_V2_HIP.local_update_group (one graph replay for the n updates)."""
        from dsac_v2_hip import HipBatchGroup

        if batch_size != self.engine.batch:
            raise ValueError("batch_size %d != the engine's minibatch rows %d" % (batch_size, self.engine.batch))
        if self.device_indices:
            # no draw here, no index on the host: "the rows the device draws at issue" for minibatches index_iteration .. + n - 1
            size, it = self._drawable_size(), self.index_iteration
            self.index_iteration += int(n)
            return HipBatchGroup(self.engine, None, drawn=(it, int(n), size, self.index_seed))
        # ONE call of shape (n, batch): the legacy RandomState fills int64 draws element by element with no buffering between
        # calls, so this is the stream of n calls of `batch` draws (values AND final generator state; tests/test_host_side.py
        # pins it, the trainer-trajectory fixtures compare every index with the reference loop's) at a quarter of the host time
        idxs = np.random.randint(0, self.size, size=(int(n), batch_size))
        return HipBatchGroup(self.engine, idxs)

    def _drawable_size(self):
        size = self.size
        if size <= 0:
            raise ValueError("cannot sample from an empty buffer (np.random.randint(0, 0) raises in the reference too)")
        return size

    def sample_batch(self, batch_size: int):
        from dsac_v2_hip import HipBatch

        if self.device_indices:
            size, it = self._drawable_size(), self.index_iteration
            self.index_iteration += 1
            self.engine.draw_indices(it, 1)   # replay_buffer.py:86 on the device ...
            self.engine.gather(None)          # ... and :87-90 from the row it drew
            return HipBatch(self.engine, None, drawn=(it, size, self.index_seed))
        idxs = np.random.randint(0, self.size, size=batch_size)  # reference replay_buffer.py:86
        self.engine.gather(idxs)
        return HipBatch(self.engine, idxs)
