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

`save(path)` / `load(path)` write and read a snapshot of the ring, format "dsact-ring-1" (DESIGN.md section 18): a directory with
one little-endian file per column -- rows [0, size) in the ring's stored form (float32, or the uint8 codes of a coded ring) --
and a meta.json holding the cursor, the shapes, the codebook's bit patterns, the per-chunk device digests and the state of the
device index draw. load() refuses a snapshot of another capacity, shape, coded-ness or codebook before it touches the ring, and
leaves the ring EMPTY when the digests the device computes over the restored rows are not the saved ones.

`save_async(path)` writes the same snapshot without holding the caller: one launch takes a consistent copy
of the live rows, with its digests, inside HBM in stream order, and a writer thread moves that copy to disk while the caller goes
on adding and sampling. It returns a RingSaveJob; the files are the ones save() would have written at the moment of the call.
"""
import json
import os
import shutil
import sys
import tempfile
import threading
import time

import numpy as np

from dsact.engine import RING_COLUMNS, DsactEngine, current_engine, ring_digest_reference

__all__ = ["HipReplayBuffer", "RingSaveJob", "parse_obs_codebook", "index_seed_from", "act_seed_from"]

MAX_CODES = 256
RING_FORMAT = "dsact-ring-1"
_M64 = (1 << 64) - 1


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


class RingSaveJob:
    """A background snapshot in flight (HipReplayBuffer.save_async). `path` is where the snapshot appears, `size` the rows it
    holds, `seconds` the writer's wall time once it is done (None before). done() asks without waiting; wait() joins the writer,
    releases the device copy and re-raises what the writer raised -- it is called on the thread that owns the buffer."""

    def __init__(self, buffer, path, info, index_seed, index_iteration, keep_shadow, on_chunk, on_done=None):
        self.path, self.size, self.seconds = path, int(info["size"]), None
        self._buffer, self._keep_shadow, self._error, self._released = buffer, keep_shadow, None, False
        eng, chunk_rows, digs = buffer.engine, int(info["chunk_rows"]), []

        def digest(r0, n):
            if not digs:
                digs.append(eng.buffer_shadow_digests())
            return tuple(int(v) for v in digs[0][r0 // chunk_rows])

        def run():
            t0 = time.perf_counter()
            try:
                buffer._write_snapshot(path, self.size, int(info["ptr"]), chunk_rows, index_seed, index_iteration,
                                       eng.buffer_shadow_export, digest, on_chunk)
                if on_done is not None:
                    on_done()
            except BaseException as e:      # (kept for wait(): a thread has nobody to raise to)
                self._error = e
            self.seconds = time.perf_counter() - t0

        # (not a daemon: an interpreter that exits with a job pending lets the snapshot finish instead of cutting it off)
        self._thread = threading.Thread(target=run, name="dsact-ring-snapshot")

    def done(self):
        return not self._thread.is_alive()

    def wait(self):
        self._thread.join()
        if not self._released:
            self._released = True
            if self._buffer._snapshot_job is self:
                self._buffer._snapshot_job = None
            self._buffer.engine.buffer_shadow_release(free=not self._keep_shadow)
        if self._error is not None:
            raise self._error
        return self.path


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
        self._snapshot_job = None     # the pending RingSaveJob of save_async, if any
        self.snapshot_waits = 0       # save_async calls that first had to wait for the one before
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

    # ---- snapshots (format "dsact-ring-1") ---------------------------------------------------------------
    def _ring_columns(self):
        """[(name, elements per row, dtype)] of the six columns in stored form"""
        o = np.dtype(np.uint8) if self.codebook is not None else np.dtype("<f4")
        f = np.dtype("<f4")
        return [("obs", self._obs_flat, o), ("obs2", self._obs_flat, o), ("act", int(self.act_dim), f), ("rew", 1, f), ("done", 1, f),
                ("logp", 1, f)]

    def _snapshot_identity(self):
        return {"capacity": int(self.max_size), "obs_shape": [int(d) for d in self._obs_shape], "act_dim": int(self.act_dim),
                "coded": self.codebook is not None,
                "codebook": None if self.codebook is None else [int(b) for b in np.ascontiguousarray(self.codebook).view(np.uint32)]}

    def save(self, path, chunk_rows=65536, overwrite=False):
        """Writes the live rows [0, size) and the cursor to the directory `path`. The rows leave HBM chunk by chunk (the host never
        holds more than `chunk_rows` rows) and each chunk's six digests are taken from the device. Everything is written into a
        temporary directory beside `path`, meta.json last, and renamed: a snapshot either exists whole or not at all. An
        existing `path` raises FileExistsError unless overwrite=True. Synchronous."""
        path = os.path.abspath(os.fspath(path))
        chunk_rows = int(chunk_rows)
        if chunk_rows < 1:
            raise ValueError("chunk_rows must be >= 1 (got %d)" % chunk_rows)
        if sys.byteorder != "little":
            raise NotImplementedError("dsact-ring-1 files are little-endian; this host is not")
        if os.path.lexists(path) and not overwrite:
            raise FileExistsError("%s exists (pass overwrite=True to replace it)" % path)
        self._wait_snapshot()
        eng = self.engine
        if hasattr(eng, "sync"):
            eng.sync()
        return self._write_snapshot(path, int(self.size), int(self.ptr), chunk_rows, int(self.index_seed), int(self.index_iteration),
                                    eng.buffer_export, eng.buffer_digest)

    def _write_snapshot(self, path, size, ptr, chunk_rows, index_seed, index_iteration, export, digest, on_chunk=None):
        """the file side of save() and of save_async()'s writer thread: `export(row0, n)` gives a chunk's columns in stored form and
        `digest(row0, n)` its six digests -- from the ring, or from the shadow of a background snapshot"""
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = tempfile.mkdtemp(prefix=os.path.basename(path) + ".tmp-", dir=os.path.dirname(path))
        try:
            files = {k: open(os.path.join(tmp, k + ".bin"), "wb") for k in RING_COLUMNS}
            chunks, total = [], [0] * 6
            try:
                for i, r0 in enumerate(range(0, size, chunk_rows)):
                    n = min(chunk_rows, size - r0)
                    cols = export(r0, n)
                    dig = digest(r0, n)
                    for k, _, dt in self._ring_columns():
                        a = np.ascontiguousarray(cols[k])
                        if a.dtype != dt:
                            raise ValueError("the engine exported column %s as %s, the stored form is %s" % (k, a.dtype, dt))
                        a.tofile(files[k])
                    chunks.append(["%016x" % v for v in dig])
                    total = [(t + v) & _M64 for t, v in zip(total, dig)]
                    if on_chunk is not None:
                        for f in files.values():
                            f.flush()
                        on_chunk(i)
            finally:
                for f in files.values():
                    f.close()
            meta = dict(self._snapshot_identity(), format=RING_FORMAT, size=size, ptr=ptr, chunk_rows=chunk_rows,
                        digests={"chunks": chunks, "total": ["%016x" % v for v in total]},
                        index_seed=index_seed, index_iteration=index_iteration)
            with open(os.path.join(tmp, "meta.json"), "w") as f:      # last: a directory without it is not a snapshot
                json.dump(meta, f, indent=1)
                f.flush()
                os.fsync(f.fileno())
            old = None
            if os.path.lexists(path):
                old = tempfile.mkdtemp(prefix=os.path.basename(path) + ".old-", dir=os.path.dirname(path))
                os.rename(path, os.path.join(old, "d"))
            os.rename(tmp, path)
            if old is not None:
                shutil.rmtree(old, ignore_errors=True)
        except BaseException:
            shutil.rmtree(tmp, ignore_errors=True)
            raise
        return path

    # ---- background snapshots ---------------------------------------------------------------------------
    def save_async(self, path, chunk_rows=65536, overwrite=False, max_bytes=None, keep_shadow=True, on_chunk=None, on_done=None):
        """save() without the wait: the files that save(path, chunk_rows, overwrite) would write AT THE MOMENT OF THIS CALL, byte
        for byte, written by a second thread while this one goes on adding and sampling. The calling thread refuses what save()
        refuses, takes ONE consistent copy of the live rows inside HBM (engine.buffer_shadow_take: one launch in stream order that
        also digests every chunk, no wait) and captures size, ptr, index_seed and index_iteration; the writer thread then exports
        the copy chunk by chunk -- the host still holds one chunk -- and writes the six column files, meta.json and the rename as
        save() does. Returns the RingSaveJob at once.
          max_bytes    refuse (DsactError) a copy that needs more device bytes than this; None: no bound
          keep_shadow  False frees the copy's device memory when the job is waited for (True keeps it for the next snapshot)
          on_chunk(i)  called on the WRITER thread after chunk i is on disk (progress reporting)
          on_done()    called on the WRITER thread once the snapshot is in place (the trainer completes its run state there);
                       what it raises is the job's error
        One job at a time: a second save_async, save(), load() and dropping the buffer first wait for a pending job
        (`snapshot_waits` counts the save_async calls that had to). job.wait() belongs to the thread that owns the buffer."""
        path = os.path.abspath(os.fspath(path))
        chunk_rows = int(chunk_rows)
        if chunk_rows < 1:
            raise ValueError("chunk_rows must be >= 1 (got %d)" % chunk_rows)
        if sys.byteorder != "little":
            raise NotImplementedError("dsact-ring-1 files are little-endian; this host is not")
        if os.path.lexists(path) and not overwrite:
            raise FileExistsError("%s exists (pass overwrite=True to replace it)" % path)
        if not callable(getattr(self.engine, "buffer_shadow_take", None)):
            raise NotImplementedError("save_async: the engine %s has no buffer_shadow_take()" % type(self.engine).__name__)
        if self._snapshot_job is not None:
            self.snapshot_waits += 1          # back-pressure: one shadow, one writer
            self._wait_snapshot()
        info = self.engine.buffer_shadow_take(chunk_rows, int(max_bytes or 0))
        job = RingSaveJob(self, path, info, int(self.index_seed), int(self.index_iteration), bool(keep_shadow), on_chunk, on_done)
        self._snapshot_job = job
        job._thread.start()
        return job

    def _wait_snapshot(self):
        """joins a pending background snapshot, releases its shadow and raises what its writer raised"""
        job = getattr(self, "_snapshot_job", None)
        if job is not None:
            job.wait()

    def __del__(self):
        try:
            self._wait_snapshot()
        except Exception:
            pass

    def _read_snapshot_meta(self, path):
        """meta.json of a snapshot this ring can take, or ValueError -- nothing here touches the ring"""
        fn = os.path.join(path, "meta.json")
        if not os.path.isfile(fn):
            raise ValueError("%s holds no meta.json: not a complete %s snapshot" % (path, RING_FORMAT))
        with open(fn) as f:
            meta = json.load(f)
        if meta.get("format") != RING_FORMAT:
            raise ValueError("%s has format %r, this is %s" % (path, meta.get("format"), RING_FORMAT))
        mine = self._snapshot_identity()
        why = {"capacity": "a ring of another capacity overwrites other rows from here on: it would not be the same run",
               "obs_shape": "another observation shape", "act_dim": "another action width",
               "coded": "a coded ring and an fp32 ring store different bytes", "codebook": "the codebook's bit patterns differ"}
        for k in ("capacity", "obs_shape", "act_dim", "coded", "codebook"):
            theirs = meta.get(k)
            if k == "obs_shape" and theirs is not None:
                theirs = [int(d) for d in theirs]
            if theirs != mine[k]:
                shown = (theirs, mine[k]) if k != "codebook" else ("...", "...")
                raise ValueError("%s: %s is %r in the snapshot and %r here (%s)" % (path, k, shown[0], shown[1], why[k]))
        size, ptr, cap, chunk = int(meta["size"]), int(meta["ptr"]), int(self.max_size), int(meta["chunk_rows"])
        if not (0 <= size <= cap and (ptr == size % cap if size < cap else 0 <= ptr < cap)) or chunk < 1:
            raise ValueError("%s: (size %d, ptr %d, chunk_rows %d) is no state a ring of %d rows reaches" % (path, size, ptr, chunk, cap))
        for k, w, dt in self._ring_columns():
            cf = os.path.join(path, k + ".bin")
            have = os.path.getsize(cf) if os.path.isfile(cf) else -1
            if have != size * w * dt.itemsize:
                raise ValueError("%s: %s.bin holds %d bytes, %d rows x %d bytes are %d" % (path, k, have, size, w * dt.itemsize,
                                                                                          size * w * dt.itemsize))
        chunks = meta.get("digests", {}).get("chunks")
        if not isinstance(chunks, list) or len(chunks) != (size + chunk - 1) // chunk or any(len(c) != 6 for c in chunks):
            raise ValueError("%s: the digest list does not cover %d rows in chunks of %d" % (path, size, chunk))
        if self.device_indices and int(meta.get("index_seed", 0)) != int(self.index_seed):
            raise ValueError("%s was drawn with index seed %#x, this buffer draws with %#x: the resumed run would sample other "
                             "minibatches" % (path, int(meta.get("index_seed", 0)), int(self.index_seed)))
        return meta

    def load(self, path):
        """Restores the snapshot at `path`: rows [0, size), the cursor and `index_iteration` (this buffer keeps its own index
        seed). Refused with ValueError BEFORE anything touches the ring: no meta.json, another format, capacity, observation shape,
        action width, coded-ness or codebook, a column file of the wrong length, another index seed while hip_device_indices is
        on. Then the rows go up chunk by chunk, and the device's digest of every chunk is compared with the file's: on a mismatch
        the ring is left EMPTY and the ValueError names the chunk and the column. Synchronous."""
        path = os.path.abspath(os.fspath(path))
        self._wait_snapshot()
        meta = self._read_snapshot_meta(path)
        eng = self.engine
        size, ptr, chunk = int(meta["size"]), int(meta["ptr"]), int(meta["chunk_rows"])
        spec = self._ring_columns()

        def read_chunk(files, n):
            return {k: np.fromfile(files[k], dtype=dt, count=n * w).reshape((n, w) if k in ("obs", "obs2", "act") else (n,))
                    for k, w, dt in spec}

        files = {k: open(os.path.join(path, k + ".bin"), "rb") for k in RING_COLUMNS}
        try:
            for r0 in range(0, size, chunk):
                eng.buffer_import(r0, read_chunk(files, min(chunk, size - r0)))
        finally:
            for f in files.values():
                f.close()
        eng.buffer_set_cursor(size, ptr)
        self.index_iteration = int(meta.get("index_iteration", 0))
        for ci, r0 in enumerate(range(0, size, chunk)):
            n = min(chunk, size - r0)
            got = tuple(eng.buffer_digest(r0, n))
            want = tuple(int(v, 16) for v in meta["digests"]["chunks"][ci])
            if got != want:
                eng.buffer_set_cursor(0, 0)
                c = next(i for i in range(6) if got[i] != want[i])
                # which side moved: the file (its bytes no longer digest to what save() recorded) or the way to HBM
                with open(os.path.join(path, RING_COLUMNS[c] + ".bin"), "rb") as f:
                    k, w, dt = spec[c]
                    f.seek(r0 * w * dt.itemsize)
                    a = np.fromfile(f, dtype=dt, count=n * w).reshape(n, w)
                cols = {kk: (a if kk == k else np.zeros((n, ww), dd)) for kk, ww, dd in spec}
                of_file = ring_digest_reference(cols, r0, [ww for _, ww, _ in spec])[c]
                raise ValueError("%s: chunk %d (rows %d .. %d), column %s: the device digests the restored rows to %016x, the snapshot "
                                 "recorded %016x (%s.bin itself digests to %016x: %s); the ring was left empty"
                                 % (path, ci, r0, r0 + n - 1, k, got[c], want[c], k, of_file,
                                    "the file changed after it was saved" if of_file != want[c] else "the rows changed on their way to the device"))
        return meta

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
