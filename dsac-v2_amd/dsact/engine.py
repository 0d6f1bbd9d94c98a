"""DsactEngine -- thin Python owner of one libdsact handle (one per GPU / process).

PyTorch-ROCm is used for exactly two things here: it OWNS the flat parameter / Adam / gradient
arenas (so `state_dict()`, `torch.save`, `torch.distributed.all_reduce` work on them unchanged), and
it provides the stream. All arithmetic of the update runs in the HIP kernels behind the C-ABI.
"""
import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _ffi
from ._ffi import DsactError
from .layout import ArenaLayout, CnnArenaLayout

STAT_KEYS = [  # order of dsact_read_stats == dsac_v2.py:188-202
    "DSAC2/critic_avg_q1-RL iter", "DSAC2/critic_avg_q2-RL iter",
    "DSAC2/critic_avg_std1-RL iter", "DSAC2/critic_avg_std2-RL iter",
    "DSAC2/critic_avg_min_std1-RL iter", "DSAC2/critic_avg_min_std2-RL iter",
    "Loss/Actor loss-RL iter", "Loss/Critic loss-RL iter",
    "DSAC2/policy_mean-RL iter", "DSAC2/policy_std-RL iter", "DSAC2/entropy-RL iter",
    "DSAC2/alpha-RL iter", "DSAC2/mean_std1", "DSAC2/mean_std2",
]


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


RING_COLUMNS = ("obs", "obs2", "act", "rew", "done", "logp")   # the ring's SoA order: digest column c = index
_M64 = (1 << 64) - 1


def ring_digest_reference(cols, row0, widths=None):
    """dsact_buffer_digest restated in NumPy uint64 arithmetic (include/dsact.h has the definition; no GPU, no library call): the
    six column sums, as Python ints, of `cols` = {obs, obs2, act, rew, done, logp} holding ring rows [row0, row0 + n) in stored
    form (float32, or uint8 codes for obs / obs2 of a coded ring). widths: (O, O, A, 1, 1, 1); None reads them off the arrays."""
    out = []
    u = np.uint64
    with np.errstate(over="ignore"):
        for c, key in enumerate(RING_COLUMNS):
            a = np.ascontiguousarray(cols[key])
            n = int(a.shape[0])
            if a.dtype == np.uint8:
                v = a.reshape(-1).astype(np.uint64)
            elif a.dtype == np.float32:
                v = a.reshape(-1).view(np.uint32).astype(np.uint64)
            else:
                raise ValueError("ring column %s must be float32 or uint8 (got %s)" % (key, a.dtype))
            w = int(widths[c]) if widths is not None else (v.size // n if n else 1)
            if v.size != n * w:
                raise ValueError("ring column %s holds %d elements, expected %d rows x %d" % (key, v.size, n, w))
            g = u((int(row0) * w) & _M64) + np.arange(v.size, dtype=np.uint64)
            x = g * u(0x9E3779B97F4A7C15) + ((u(c + 1) << u(32)) | v)
            x ^= x >> u(30)
            x *= u(0xBF58476D1CE4E5B9)
            x ^= x >> u(27)
            x *= u(0x94D049BB133111EB)
            x ^= x >> u(31)
            out.append(int(x.sum(dtype=np.uint64)) & _M64)
    return tuple(out)


class DsactEngine:
    def __init__(self, obs_dim: int, act_dim: int, hidden: Sequence[int], batch: int, *,
                 gamma=0.99, tau=0.005, tau_b=None, auto_alpha=True, alpha=0.2, delay_update=2,
                 lr_q=1e-4, lr_pi=1e-4, lr_alpha=3e-4, min_log_std=-20.0, max_log_std=0.5,
                 global_batch: Optional[int] = None, device: int = 0, conv_type: Optional[str] = None,
                 algo: str = "DSAC_V2", td_bound: float = 20.0, v1_bound: bool = True, value_act: int = 0, policy_act: int = 0, act_dist: int = 0,
                 policy_std_type: str = "mlp_shared", value_out_act: int = 0, policy_out_act: int = 0,
                 policy_hidden: Optional[Sequence[int]] = None, pad_widths: bool = False, cnn_act: bool = False):
        """obs_dim: int for the MLP nets; with `conv_type` ("type_1" / "type_2", reference
        networks/cnn.py:173-228) the (C, H, W) image shape, and `hidden` must be that type's MLP widths.

        cnn_act: with `conv_type`, enable the CNN acting path (enable_cnn_acting). Nothing for MLP nets.

        pad_widths (round 6): hidden widths the row-slice chain kernels do not take as they are -- ragged ones (96, 40), unequal
        value / policy lists of the same depth -- are STORED zero-padded to one common width of 64 / 128 / 256 when that puts
        the update on the chains (ArenaLayout pad_to: the reference's tensors are windows of the stored ones, the padding stays an
        exact zero). Falls back to the exact layout (tile-stage kernels) when the chains refuse the padded shape anyway."""
        kw = dict(gamma=gamma, tau=tau, tau_b=tau_b, auto_alpha=auto_alpha, alpha=alpha, delay_update=delay_update, lr_q=lr_q, lr_pi=lr_pi,
                  lr_alpha=lr_alpha, min_log_std=min_log_std, max_log_std=max_log_std, global_batch=global_batch, device=device,
                  conv_type=conv_type, algo=algo, td_bound=td_bound, v1_bound=v1_bound, value_act=value_act, policy_act=policy_act,
                  act_dist=act_dist, policy_std_type=policy_std_type, value_out_act=value_out_act, policy_out_act=policy_out_act,
                  policy_hidden=policy_hidden)
        pad = self._pad_width(hidden, policy_hidden, batch, obs_dim, **{k: v for k, v in kw.items() if k != "policy_hidden"}) if pad_widths else None
        self._init(obs_dim, act_dim, hidden, batch, pad_to=pad, **kw)
        if pad and not self.chain_active:     # the chains refused it (LDS, an environment switch, ...): no reason to carry the padding
            self.close()
            self._init(obs_dim, act_dim, hidden, batch, pad_to=None, **kw)
        if cnn_act and self.conv_type:
            self.enable_cnn_acting()

    def enable_cnn_acting(self):
        """dsact_cnn_acting_enable: from now on act_sample / act_sample_batch and behaviour_hold serve this CNN engine (frames
        as [n, C, H, W] or [n, O] rows). Allocates the path's buffers; idempotent. Raises DsactError on an MLP engine."""
        self._chk(self._lib.dsact_cnn_acting_enable(self._h))
        self.cnn_act = True

    def cnn_acting_capture(self):
        """dsact_cnn_acting_capture(on=1): the device-resident acting calls of this CNN engine (act_sample_device_counted,
        act_mode_device) become legal while the engine's stream is captured into a graph. They record no
        event any more; a held act_sample_batch records its fence itself, behind everything enqueued on the engine's stream.
        Needs enable_cnn_acting first; sticky (it cannot be switched off); idempotent."""
        self._chk(self._lib.dsact_cnn_acting_capture(self._h, 1))

    @staticmethod
    def _pad_width(hidden, policy_hidden, batch, obs_dim, *, conv_type=None, algo="DSAC_V2", policy_std_type="mlp_shared", value_act=0,
                   policy_act=0, **_):
        """the common stored width that puts this configuration on the row-slice chains, or None (no padding needed / possible):
        the shape conditions of dsact_create's chain_ok (csrc/dsact_api.hip) + act(0) == 0 for both hidden activations"""
        ph = list(policy_hidden) if policy_hidden is not None else list(hidden)
        widths = list(hidden) + ph
        if conv_type or policy_std_type == "mlp_separated" or len(ph) != len(hidden) or len(hidden) > 4:
            return None
        if len(set(widths)) == 1 and widths[0] in (64, 128, 256):
            return None                                   # the chains take it as it is
        if max(widths) > 256 or 4 in (int(value_act), int(policy_act)):   # 4 = sigmoid: act(0) = 0.5 would make the padding live
            return None
        if batch % 16 or (batch > 256 and batch % 256):
            return None
        return 64 if max(widths) <= 64 else (128 if max(widths) <= 128 else 256)

    def _init(self, obs_dim, act_dim, hidden, batch, *, pad_to=None,
              gamma=0.99, tau=0.005, tau_b=None, auto_alpha=True, alpha=0.2, delay_update=2,
              lr_q=1e-4, lr_pi=1e-4, lr_alpha=3e-4, min_log_std=-20.0, max_log_std=0.5,
              global_batch=None, device=0, conv_type=None,
              algo="DSAC_V2", td_bound=20.0, v1_bound=True, value_act=0, policy_act=0, act_dist=0,
              policy_std_type="mlp_shared", value_out_act=0, policy_out_act=0, policy_hidden=None):
        import torch

        self._lib = _ffi.load()
        if not torch.cuda.is_available():
            raise DsactError("DsactEngine needs an MI355X (torch.cuda.is_available() is False); "
                             "the DSAC-T update has no CPU fallback")
        self.torch = torch
        self.conv_type = conv_type
        self.cnn_act = False
        self.algo = algo
        if algo not in ("DSAC_V2", "DSAC_V1"):
            raise DsactError("algo must be DSAC_V2 or DSAC_V1")
        if conv_type and policy_std_type != "mlp_shared":
            raise DsactError("policy_std_type %r is built for the MLP nets only" % policy_std_type)
        if conv_type:
            self.layout = CnnArenaLayout(obs_dim, act_dim, conv_type, n_critics=2 if algo == "DSAC_V2" else 1)
            if list(hidden) != self.layout.hidden:
                raise DsactError("conv_type %s fixes the MLP widths to %s" % (conv_type, self.layout.hidden))
            self.obs_shape = self.layout.obs_shape
            obs_dim = self.layout.obs_dim
        else:
            self.layout = ArenaLayout(obs_dim, act_dim, list(hidden), n_critics=2 if algo == "DSAC_V2" else 1,
                                      policy_std_type=policy_std_type, policy_hidden=policy_hidden, pad_to=pad_to)
            self.obs_shape = (int(obs_dim),)
        self.obs_dim, self.act_dim, self.batch = int(obs_dim), int(act_dim), int(batch)
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        cfg = _ffi.Config()
        cfg.obs_dim, cfg.act_dim, cfg.n_hidden = obs_dim, act_dim, len(hidden)
        if len(hidden) > _ffi.MAX_HIDDEN:
            raise DsactError("at most %d hidden layers" % _ffi.MAX_HIDDEN)
        for i, w in enumerate(hidden):
            cfg.hidden[i] = int(pad_to or w)      # (pad_to: the library sees the STORED widths -- an equal-width configuration)
        cfg.batch = batch
        cfg.global_batch = int(global_batch or batch)
        cfg.auto_alpha = 1 if auto_alpha else 0
        cfg.delay_update = int(delay_update)
        cfg.gamma, cfg.tau = gamma, tau
        cfg.tau_b = tau if tau_b is None else tau_b
        cfg.lr_q, cfg.lr_pi, cfg.lr_alpha = lr_q, lr_pi, lr_alpha
        cfg.alpha_fixed = alpha
        cfg.min_log_std, cfg.max_log_std = min_log_std, max_log_std
        cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps = 0.9, 0.999, 1e-8
        if conv_type:
            cfg.conv_type = self.layout.conv_id
            cfg.img_c, cfg.img_h, cfg.img_w = self.obs_shape
        cfg.algo = 0 if algo == "DSAC_V2" else 1
        cfg.td_bound = float(td_bound)
        cfg.v1_unbounded = 0 if v1_bound else 1
        cfg.value_act, cfg.policy_act = int(value_act), int(policy_act)   # hidden activations: 0 gelu .. 5 tanh (include/dsact.h)
        cfg.policy_std_param = 1 if policy_std_type == "parameter" else 0   # networks/mlp.py:63-73 (include/dsact.h)
        cfg.policy_twin = 1 if policy_std_type == "mlp_separated" else 0    # networks/mlp.py:46-57: two MLPs side by side
        if policy_hidden is not None and list(policy_hidden) != list(hidden) and not pad_to:   # value_hidden_sizes != policy_hidden_sizes (include/dsact.h)
            if conv_type or not 1 <= len(policy_hidden) <= _ffi.MAX_HIDDEN:
                raise DsactError("policy_hidden needs the MLP nets and 1..%d layers" % _ffi.MAX_HIDDEN)
            for i, w in enumerate(policy_hidden):
                cfg.policy_hidden[i] = int(w)
            if len(policy_hidden) != len(hidden):    # lists of different depth (include/dsact.h policy_n_hidden)
                cfg.policy_n_hidden = len(policy_hidden)
        cfg.value_out_act, cfg.policy_out_act = int(value_out_act), int(policy_out_act)   # 0 linear, 1..5 relu .. tanh (include/dsact.h)
        cfg.act_dist = int(act_dist)                                       # 0 TanhGaussDistribution, 1 GaussDistribution
        self.cfg = cfg
        self._h = C.c_void_p()
        rc = self._lib.dsact_create(C.byref(cfg), self.device_index, C.byref(self._h))
        if rc != 0:
            msg = self._lib.dsact_last_error(self._h).decode() if self._h else ""
            if self._h:
                self._lib.dsact_destroy(self._h)
                self._h = C.c_void_p()
            raise DsactError("dsact_create failed (%s): %s" % (_ffi.E_NAMES.get(rc, rc), msg))
        lay = self.layout
        assert self._lib.dsact_online_count(self._h) == lay.n_online, (self._lib.dsact_online_count(self._h), lay.n_online)
        assert self._lib.dsact_target_count(self._h) == lay.n_target
        assert self._lib.dsact_q_count(self._h) == lay.n_q and self._lib.dsact_pi_count(self._h) == lay.n_pi
        # arenas: torch tensors, device pointers handed to the library
        dev = self.device
        self.online = torch.zeros(lay.n_online, dtype=torch.float32, device=dev)
        self.target = torch.zeros(lay.n_target, dtype=torch.float32, device=dev)
        self.adam_m = torch.zeros(lay.n_online, dtype=torch.float32, device=dev)
        self.adam_v = torch.zeros(lay.n_online, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(lay.n_online + 2, dtype=torch.float32, device=dev)
        self._chk(self._lib.dsact_bind_arenas(
            self._h, self.online.data_ptr(), self.target.data_ptr(), self.adam_m.data_ptr(),
            self.adam_v.data_ptr(), self.grads.data_ptr()))
        self._graph_steps = 0
        self.stage_serial = 0
        self.buffer_capacity = 0
        self.buffer_coded = False
        self.rows_added = 0      # rows ever written to the ring (HipBatch tokens detect overwritten rows with it)
        self.fill_epoch = 0      # bumped by buffer_fill_device (writes at an arbitrary row: outstanding tokens become invalid)
        self.index_seed = 0      # set_index_rng: 0 = the replay indices are the caller's host draws

    # ---- plumbing -----------------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise DsactError("%s: %s" % (_ffi.E_NAMES.get(rc, rc), self._lib.dsact_last_error(self._h).decode()))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dsact_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_torch_stream(self):
        """Run on torch's current stream. The legacy default stream has no handle to pass (its `cuda_stream` is 0,
        which `dsact_set_stream` reads as "handle-owned stream"): enter a `torch.cuda.stream(...)` context first, or --
        simpler -- leave the engine on its own stream and issue the torch work on `engine.torch_stream`."""
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        if not s:
            raise DsactError("torch's current stream is the legacy default stream (handle 0); run torch work under "
                             "`with torch.cuda.stream(engine.torch_stream):` instead")
        self._chk(self._lib.dsact_set_stream(self._h, C.c_void_p(s)))
        self._torch_stream = None

    @property
    def stream_ptr(self) -> int:
        return int(self._lib.dsact_get_stream(self._h) or 0)

    @property
    def torch_stream(self):
        """The engine's HIP stream as a torch stream: torch ops issued under `torch.cuda.stream(engine.torch_stream)`
        (collectives on `engine.grads`, tensor math on the arenas) are stream-ordered with the engine's kernels."""
        ts = getattr(self, "_torch_stream", None)
        if ts is None or ts.cuda_stream != self.stream_ptr:
            ts = self.torch.cuda.ExternalStream(self.stream_ptr, device=self.device)
            self._torch_stream = ts
        return ts

    def sync(self):
        self._chk(self._lib.dsact_sync(self._h))

    def set_action_limits(self, high, low):
        hi, lo = _f32(high), _f32(low)
        self._chk(self._lib.dsact_set_action_limits(self._h, _ffi.fptr(hi), _ffi.fptr(lo)))
        self.act_high, self.act_low = hi.reshape(-1).copy(), lo.reshape(-1).copy()   # (what act_sample_device clips to)

    # ---- state ------------------------------------------------------------------------------------
    def get_state(self):
        steps = (C.c_int32 * 3)()
        ms = (C.c_float * 2)()
        self._chk(self._lib.dsact_get_state(self._h, steps, ms))
        return {"adam_steps": [int(s) for s in steps], "mean_std": [float(ms[0]), float(ms[1])]}

    def set_state(self, adam_steps=None, mean_std=None):
        st = (C.c_int32 * 3)(*adam_steps) if adam_steps is not None else None
        ms = (C.c_float * 2)(*mean_std) if mean_std is not None else None
        self._chk(self._lib.dsact_set_state(self._h, st, ms))

    HYPER = {"gamma": 0, "tau": 1, "tau_b": 2, "auto_alpha": 3, "alpha": 4, "delay_update": 5, "TD_bound": 6, "bound": 7}

    def set_hyper(self, name: str, value):
        """dsact_set_hyper: the next enqueued update uses `value`; a captured graph is dropped (build it again)"""
        self._chk(self._lib.dsact_set_hyper(self._h, self.HYPER[name], float(value)))
        self._graph_steps = 0

    # ---- replay ring -------------------------------------------------------------------------------
    def buffer_create(self, capacity: int, codebook=None):
        """codebook: None (fp32 ring) or the validated float32 table of a coded image ring (dsact_buffer_create_coded)"""
        if codebook is None:
            self._chk(self._lib.dsact_buffer_create(self._h, int(capacity)))
        else:
            book = np.ascontiguousarray(codebook, dtype=np.float32)
            self._chk(self._lib.dsact_buffer_create_coded(self._h, int(capacity), _ffi.fptr(book), int(book.shape[0])))
        self.buffer_capacity = int(capacity)
        self.buffer_coded = codebook is not None
        self.codebook = None if codebook is None else book     # (byte frames of a tensor environment decode through it)

    # ---- ring snapshots: stored form out of / into HBM, the cursor, the device-side digest. Synchronous. ---
    ring_digest_reference = staticmethod(ring_digest_reference)

    @property
    def ring_widths(self):
        """(O, O, A, 1, 1, 1): elements per row of the six ring columns"""
        return (self.obs_dim, self.obs_dim, self.act_dim, 1, 1, 1)

    def _ring_dtypes(self):
        o = np.uint8 if getattr(self, "buffer_coded", False) else np.float32
        return (o, o, np.float32, np.float32, np.float32, np.float32)

    def buffer_export(self, row0: int, n: int) -> Dict[str, np.ndarray]:
        """dsact_buffer_export: ring rows [row0, row0 + n) in stored form -- {obs, obs2: [n, O] float32 (uint8 codes on a coded
        ring), act: [n, A], rew, done, logp: [n]}. row0 + n <= buffer_size (DsactError otherwise)."""
        rows = max(int(n), 0)
        out = {k: np.empty((rows, w) if i < 3 else (rows,), dt)
               for i, (k, w, dt) in enumerate(zip(RING_COLUMNS, self.ring_widths, self._ring_dtypes()))}
        self._chk(self._lib.dsact_buffer_export(self._h, int(row0), int(n), *[a.ctypes.data_as(C.c_void_p) for a in out.values()]))
        return out

    def buffer_import(self, row0: int, cols):
        """dsact_buffer_import: writes ring rows [row0, row0 + n) from `cols` in stored form (buffer_export's dict; n = rows of
        `rew`); row0 + n <= capacity. Moves neither size nor ptr (buffer_set_cursor). Counts as a write at an arbitrary row:
        outstanding HipBatch / HipBatchGroup tokens re-gather or raise as after buffer_fill_device."""
        n = int(np.shape(cols["rew"])[0])
        arrs = []
        for i, (k, w, dt) in enumerate(zip(RING_COLUMNS, self.ring_widths, self._ring_dtypes())):
            a = np.asarray(cols[k])
            if a.dtype != dt:
                raise ValueError("ring column %s must have dtype %s (got %s)" % (k, np.dtype(dt).name, a.dtype))
            if a.size != n * w:
                raise ValueError("ring column %s holds %d elements, expected %d rows x %d" % (k, a.size, n, w))
            arrs.append(np.ascontiguousarray(a))
        self._chk(self._lib.dsact_buffer_import(self._h, int(row0), n, *[a.ctypes.data_as(C.c_void_p) for a in arrs]))
        self.fill_epoch += 1

    def buffer_set_cursor(self, size: int, ptr: int):
        """dsact_buffer_set_cursor: size and ptr, one of the states the reference's store() reaches (DsactError otherwise)"""
        self._chk(self._lib.dsact_buffer_set_cursor(self._h, int(size), int(ptr)))
        self.fill_epoch += 1     # (the tokens' bookkeeping is relative to the cursor they were sampled at)

    def buffer_digest(self, row0: int = 0, n: Optional[int] = None):
        """dsact_buffer_digest: the six 64-bit column digests of ring rows [row0, row0 + n) as Python ints, computed on the
        device (n None: up to buffer_size). Equals ring_digest_reference(buffer_export(row0, n), row0)."""
        if n is None:
            n = self.buffer_size - int(row0)
        out = (C.c_uint64 * 6)()
        self._chk(self._lib.dsact_buffer_digest(self._h, int(row0), int(n), out))
        return tuple(int(v) for v in out)

    # ---- background snapshots: take / release on the owning thread, export / digests on ONE other thread ---
    def buffer_shadow_take(self, chunk_rows: int, max_bytes: int = 0) -> Dict[str, int]:
        """dsact_buffer_shadow_take: a consistent device copy of ring rows [0, buffer_size) with the digests of its chunks, in
        stream order and without a wait. Returns what was captured: {size, ptr, chunk_rows, n_chunks, bytes}. Rows added after
        the call do not reach the copy. max_bytes 0: no bound. One shadow at a time (DsactError until buffer_shadow_release)."""
        info = _ffi.ShadowInfo()
        self._chk(self._lib.dsact_buffer_shadow_take(self._h, int(chunk_rows), int(max_bytes or 0), C.byref(info)))
        self._shadow_info = {k: int(getattr(info, k)) for k in ("size", "ptr", "chunk_rows", "n_chunks", "bytes")}
        return dict(self._shadow_info)

    def _chk_shadow(self, rc):
        if rc != 0:   # the reader calls keep their own error text: dsact_last_error belongs to the owning thread
            raise DsactError("%s: %s" % (_ffi.E_NAMES.get(rc, rc), self._lib.dsact_buffer_shadow_error(self._h).decode()))

    def buffer_shadow_export(self, row0: int, n: int) -> Dict[str, np.ndarray]:
        """dsact_buffer_shadow_export: rows [row0, row0 + n) of the shadow in buffer_export's form. Callable from one other
        thread while the owning thread goes on using the engine; waits for the take only."""
        rows = max(int(n), 0)
        out = {k: np.empty((rows, w) if i < 3 else (rows,), dt)
               for i, (k, w, dt) in enumerate(zip(RING_COLUMNS, self.ring_widths, self._ring_dtypes()))}
        self._chk_shadow(self._lib.dsact_buffer_shadow_export(self._h, int(row0), int(n), *[a.ctypes.data_as(C.c_void_p) for a in out.values()]))
        return out

    def buffer_shadow_digests(self) -> np.ndarray:
        """dsact_buffer_shadow_digests: uint64 [n_chunks, 6] -- row k is buffer_digest(k * chunk_rows, rows of chunk k) as it was
        at the take. Reader side, like buffer_shadow_export."""
        n = int(getattr(self, "_shadow_info", {}).get("n_chunks", 0))
        out = np.zeros((n, 6), np.uint64)
        self._chk_shadow(self._lib.dsact_buffer_shadow_digests(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n))
        return out

    def buffer_shadow_release(self, free: bool = False):
        """dsact_buffer_shadow_release: owning thread, after the reader is done; free=True also frees the shadow's device memory"""
        self._chk(self._lib.dsact_buffer_shadow_release(self._h, 1 if free else 0))

    def buffer_check(self):
        """dsact_buffer_check: drains the stream; raises if a value missing from the codebook was written"""
        self._chk(self._lib.dsact_buffer_check(self._h))

    @property
    def buffer_bytes(self):
        return int(self._lib.dsact_buffer_bytes(self._h))

    def buffer_add(self, obs, act, rew, obs2, done, logp=None):
        obs, act, rew, obs2, done = _f32(obs), _f32(act), _f32(rew), _f32(obs2), _f32(done)
        n = int(rew.shape[0])
        lp = _f32(logp) if logp is not None else None
        self._chk(self._lib.dsact_buffer_add(self._h, n, _ffi.fptr(obs), _ffi.fptr(act), _ffi.fptr(rew),
                                             _ffi.fptr(obs2), _ffi.fptr(done), _ffi.fptr(lp)))
        self.rows_added += n

    def buffer_fill_device(self, row0, obs, act, rew, obs2, done):
        """rows from torch CUDA tensors (synthetic benchmark buffers stay on the device)."""
        n = int(rew.shape[0])
        for t in (obs, act, rew, obs2, done):
            assert t.is_cuda and t.dtype == self.torch.float32 and t.is_contiguous()
        self.torch.cuda.current_stream(self.device).synchronize()
        self._chk(self._lib.dsact_buffer_fill_device(self._h, int(row0), n, obs.data_ptr(), act.data_ptr(),
                                                     rew.data_ptr(), obs2.data_ptr(), done.data_ptr()))
        self.rows_added += n
        self.fill_epoch += 1

    @property
    def buffer_size(self):
        return int(self._lib.dsact_buffer_size(self._h))

    @property
    def buffer_ptr(self):
        return int(self._lib.dsact_buffer_ptr(self._h))

    def gather(self, idx):
        """idx None: row 0 of the index table as draw_indices left it (dsact_gather with idx_host == NULL)"""
        if idx is None:
            self._chk(self._lib.dsact_gather(self._h, None, self.batch))
        else:
            idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64))
            self._chk(self._lib.dsact_gather(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), int(idx.shape[0])))
        self.stage_serial += 1   # which minibatch sits in the staging set (HipBatch tokens compare against it)

    def read_batch(self, with_logp=True) -> Dict[str, np.ndarray]:
        B, O, A = self.batch, self.obs_dim, self.act_dim
        shp = (B,) + tuple(self.obs_shape)
        out = {"obs": np.empty(shp, np.float32), "act": np.empty((B, A), np.float32),
               "rew": np.empty(B, np.float32), "obs2": np.empty(shp, np.float32),
               "done": np.empty(B, np.float32)}
        lp = np.empty(B, np.float32) if with_logp else None
        self._chk(self._lib.dsact_read_batch(self._h, _ffi.fptr(out["obs"]), _ffi.fptr(out["act"]),
                                             _ffi.fptr(out["rew"]), _ffi.fptr(out["obs2"]),
                                             _ffi.fptr(out["done"]), _ffi.fptr(lp)))
        if with_logp:
            out["logp"] = lp
        return out

    def _src(self, a, n):
        """float* for dsact_load_batch: a CUDA tensor on this engine's GPU is passed by device address (no trip
        through the host), anything else as a contiguous host float32 array. Returns (pointer, keep-alive)."""
        torch = self.torch
        if isinstance(a, torch.Tensor) and a.is_cuda and a.device.index == self.device_index:
            t = a.detach().to(torch.float32).contiguous()
            assert t.numel() == n, (tuple(t.shape), n)
            return C.cast(C.c_void_p(t.data_ptr()), _ffi._FP), t
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = _f32(a)
        assert a.size == n, (a.shape, n)
        return _ffi.fptr(a), a

    def load_batch(self, obs, act, rew, obs2, done):
        """Stage a minibatch that lives outside the HIP ring: numpy / CPU tensors or CUDA tensors (mixed is fine)."""
        torch, B = self.torch, self.batch
        srcs = [self._src(obs, B * self.obs_dim), self._src(act, B * self.act_dim), self._src(rew, B),
                self._src(obs2, B * self.obs_dim), self._src(done, B)]
        if any(isinstance(k, torch.Tensor) for _, k in srcs):
            torch.cuda.current_stream(self.device).synchronize()   # the producers of the CUDA sources have finished
        self._chk(self._lib.dsact_load_batch(self._h, *[p for p, _ in srcs]))
        self.stage_serial += 1

    def upload_index_table(self, idx):
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64))
        assert idx.ndim == 2 and idx.shape[1] == self.batch
        self._chk(self._lib.dsact_upload_index_table(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     int(idx.shape[0])))

    # ---- device-side index draw (opt-in; replaces the np.random.randint of reference replay_buffer.py:86) --------------
    def set_index_rng(self, seed: int):
        """dsact_set_index_rng: Philox key of the device-side index draw; 0 switches it off (the default)"""
        self._chk(self._lib.dsact_set_index_rng(self._h, int(seed)))
        self.index_seed = int(seed)

    def draw_indices(self, first_iteration: int, n: int = 1):
        """dsact_draw_indices: rows [0, n) of the index table <- the draws of iterations first_iteration .. + n - 1 over the
        current ring size. Asynchronous."""
        self._chk(self._lib.dsact_draw_indices(self._h, int(first_iteration), int(n)))

    def read_indices(self, rows: int = 1) -> np.ndarray:
        """dsact_read_indices: the first `rows` rows of the index table, int64 [rows][batch]. Synchronous."""
        out = np.empty((int(rows), self.batch), np.int64)
        self._chk(self._lib.dsact_read_indices(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), int(rows)))
        return out

    # ---- noise ---------------------------------------------------------------------------------------
    def set_noise(self, eps_new, eps_2, z5, z6):
        a, b, c, d = _f32(eps_new), _f32(eps_2), _f32(z5), _f32(z6)
        assert a.shape == (self.batch, self.act_dim) and c.shape == (self.batch,)
        self._chk(self._lib.dsact_set_noise(self._h, _ffi.fptr(a), _ffi.fptr(b), _ffi.fptr(c), _ffi.fptr(d)))

    def set_device_rng(self, seed: int):
        self._chk(self._lib.dsact_set_device_rng(self._h, int(seed)))

    # ---- update ---------------------------------------------------------------------------------------
    def compute_grads(self, iteration: int, flags: int = 0):
        self._chk(self._lib.dsact_compute_grads(self._h, int(iteration), int(flags)))

    def apply_update(self, iteration: int):
        self._chk(self._lib.dsact_apply_update(self._h, int(iteration)))

    def step(self, iteration: int, flags: int = 0):
        self._chk(self._lib.dsact_step(self._h, int(iteration), int(flags)))

    def graph_build(self, steps_per_graph: int = 2, flags: int = 0):
        self._chk(self._lib.dsact_graph_build(self._h, int(steps_per_graph), int(flags)))
        self._graph_steps = int(steps_per_graph)

    def graph_run(self, first_iteration: int, n_steps: int):
        self.stage_serial += 1   # the index table's device-side gather replaces the staged minibatch
        self._chk(self._lib.dsact_graph_run(self._h, int(first_iteration), int(n_steps)))

    def run_group(self, first_iteration: int, idx_rows, noise_rows=None, flags: int = 0, n: int = None):
        """dsact_run_group: len(idx_rows) x { sample_batch -> local_update } of the reference's loop between two sampler calls
        as one graph replay. idx_rows int64 [n][batch] (drawn by the caller with the reference's np.random.randint calls), or
        None with `n` given: the device draws the rows of those n iterations itself (set_index_rng; NULL crosses the C-ABI);
        noise_rows float32 [n][2*B*A + 2*B] (eps_new | eps_2 | z5 | z6 per update) or None for device Philox noise.
        Asynchronous."""
        if idx_rows is None:
            if n is None or int(n) < 1:
                raise ValueError("run_group(idx_rows=None) needs n, the number of updates the device draws indices for")
            n, idx_ptr = int(n), None
        else:
            idx = np.ascontiguousarray(np.asarray(idx_rows, dtype=np.int64))
            assert idx.ndim == 2 and idx.shape[1] == self.batch, idx.shape
            assert n is None or int(n) == idx.shape[0], (n, idx.shape)
            n, idx_ptr = int(idx.shape[0]), idx.ctypes.data_as(C.POINTER(C.c_int64))
        nz = None
        if noise_rows is not None:
            nz = _f32(noise_rows)
            assert nz.shape == (n, 2 * self.batch * self.act_dim + 2 * self.batch), nz.shape
        self.stage_serial += 1   # the group's last minibatch replaces the staged one
        self._chk(self._lib.dsact_run_group(self._h, int(first_iteration), n, idx_ptr, _ffi.fptr(nz), int(flags)))
        self._graph_steps = n

    # data-parallel halves (iteration and index-table row come from device state)
    def dp_begin(self, first_iteration: int):
        self._chk(self._lib.dsact_dp_begin(self._h, int(first_iteration)))

    def dp_grads(self, flags: int = 0):
        self.stage_serial += 1   # the index table's device-side gather replaces the staged minibatch
        self._chk(self._lib.dsact_dp_enqueue_grads(self._h, int(flags)))

    def dp_grads_critic(self, flags: int = 0):
        """first half of dp_grads: afterwards grads[:2*n_q] (q1 | q2) is final"""
        self.stage_serial += 1   # the index table's device-side gather replaces the staged minibatch
        self._chk(self._lib.dsact_dp_enqueue_grads_critic(self._h, int(flags)))

    def dp_grads_actor(self, flags: int = 0):
        self._chk(self._lib.dsact_dp_enqueue_grads_actor(self._h, int(flags)))

    @property
    def critic_grad_count(self):
        return 2 * self.layout.n_q

    def dp_set_strict(self, enable: bool = True):
        """strict data-parallel mode: `std_sums` (2 floats, torch-owned) is all-reduced by the caller between
        dp_forward() and dp_backward()"""
        if enable:
            self.std_sums = self.torch.zeros(2, dtype=self.torch.float32, device=self.device)
            self._chk(self._lib.dsact_dp_set_strict(self._h, self.std_sums.data_ptr()))
        else:
            self._chk(self._lib.dsact_dp_set_strict(self._h, None))
            self.std_sums = None

    def dp_forward(self, flags: int = 0):
        self.stage_serial += 1   # the index table's device-side gather replaces the staged minibatch
        self._chk(self._lib.dsact_dp_enqueue_forward(self._h, int(flags)))

    def dp_backward(self, flags: int = 0):
        self._chk(self._lib.dsact_dp_enqueue_backward(self._h, int(flags)))

    def dp_apply(self):
        self._chk(self._lib.dsact_dp_enqueue_apply(self._h))

    # native collective: RCCL opened by the library itself (the copy torch ships, so one RCCL serves the process)
    @staticmethod
    def _rccl_path():
        import torch

        p = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        return p.encode() if os.path.exists(p) else None

    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * 128)()
        rc = self._lib.dsact_comm_unique_id(self._rccl_path(), buf)
        if rc != 0:
            raise DsactError("dsact_comm_unique_id failed (%s)" % _ffi.E_NAMES.get(rc, rc))
        return bytes(buf)

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == 128
        buf = (C.c_uint8 * 128)(*unique_id)
        self._chk(self._lib.dsact_comm_init(self._h, int(rank), int(world), buf, self._rccl_path()))
        self.comm_world = int(world)

    def comm_destroy(self):
        self._chk(self._lib.dsact_comm_destroy(self._h))

    def dp_allreduce(self):
        """average of the gradient arena (+ mean_std tail) over the ranks, on the engine's stream (RCCL)"""
        self._chk(self._lib.dsact_dp_enqueue_allreduce(self._h))

    STATS_SLOTS = 16

    def stats_snapshot(self, slot: int):
        """asynchronous: reduce the last update's statistics into ring slot `slot` (read later with read_stats(slot))"""
        self._chk(self._lib.dsact_stats_snapshot(self._h, int(slot) % self.STATS_SLOTS))

    def read_stats(self, slot=None) -> Dict[str, float]:
        out = (C.c_float * 16)()
        if slot is None:
            self._chk(self._lib.dsact_read_stats(self._h, out))
        else:
            self._chk(self._lib.dsact_stats_read(self._h, int(slot) % self.STATS_SLOTS, out))
        d = {k: float(out[i]) for i, k in enumerate(STAT_KEYS)}
        d["_iteration"] = float(out[14])
        d["_device_ms"] = float(out[15]) if slot is None else -1.0   # stream time of the last eager update (-1: unknown)
        return d

    # ---- measurement ------------------------------------------------------------------------------------
    def time_steps(self, first_iteration: int, n_steps: int, use_graph: bool = True, flags: int = 0) -> float:
        ms = C.c_float()
        self.stage_serial += 1   # the index table's device-side gather replaces the staged minibatch
        self._chk(self._lib.dsact_time_steps(self._h, int(first_iteration), int(n_steps), int(flags),
                                             1 if use_graph else 0, C.byref(ms)))
        return float(ms.value)

    def time_stage(self, stage: int, reps: int = 200):
        """(milliseconds for `reps` launches, multiply-accumulates per launch) of one forward tile stage"""
        ms, macs = C.c_float(), C.c_double()
        self._chk(self._lib.dsact_time_stage(self._h, int(stage), int(reps), C.byref(ms), C.byref(macs)))
        return float(ms.value), float(macs.value)

    @property
    def chain_active(self) -> bool:
        """True when this engine runs the update as row-slice fused chains (csrc/dsact_chain.h)"""
        return bool(self._lib.dsact_chain_active(self._h))

    def profile_step(self, iteration: int, flags: int = 0):
        arr = (_ffi.KernelTime * 128)()
        n = C.c_int32()
        self.stage_serial += 1   # the index table's device-side gather replaces the staged minibatch
        self._chk(self._lib.dsact_profile_step(self._h, int(iteration), int(flags), arr, 128, C.byref(n)))
        return [(arr[i].name.decode(), float(arr[i].ms), int(arr[i].blocks)) for i in range(n.value)]

    def profile_steps(self, first_iteration: int, n_steps: int, flags: int = 0):
        """per-dispatch (name, ms, blocks) of n_steps updates issued eagerly as the sequence graph_build(n_steps) would
        capture (the pipelined one where eligible)"""
        arr = (_ffi.KernelTime * 512)()
        n = C.c_int32()
        self.stage_serial += 1
        self._chk(self._lib.dsact_profile_steps(self._h, int(first_iteration), int(n_steps), int(flags), arr, 512, C.byref(n)))
        return [(arr[i].name.decode(), float(arr[i].ms), int(arr[i].blocks)) for i in range(n.value)]

    def debug_read(self, name: str, cap: int = 1 << 24) -> np.ndarray:
        buf = np.empty(cap, np.float32)
        n = C.c_size_t()
        self._chk(self._lib.dsact_debug_read(self._h, name.encode(), _ffi.fptr(buf), cap, C.byref(n)))
        return buf[: n.value].copy()

    def debug_set(self, name: str, value: float):
        self._chk(self._lib.dsact_debug_set(self._h, name.encode(), float(value)))
        if name in ("withhold_flag", "fwd_merge"):
            self._graph_steps = 0   # the library dropped the captured graph

    def debug_get(self, name: str) -> float:
        v = C.c_double()
        self._chk(self._lib.dsact_debug_get(self._h, name.encode(), C.byref(v)))
        return float(v.value)

    def policy_dirty(self):
        """the caller wrote policy parameters with torch ops on the arena (load_state_dict, a manual copy_): the host-side
        acting snapshot (csrc/dsact_host_act.h) is refreshed before the next acting call"""
        self._chk(self._lib.dsact_debug_set(self._h, b"policy_dirty", 1.0))

    def note_torch_writes(self, params):
        """torch bumps a tensor's version counter on every in-place write: a changed sum over the policy's parameters and
        the online arena itself (slice writes through `engine.online`; the parameters are re-homed with `p.data = view`, so
        they do not share its counter) since the last look means somebody wrote them outside the library. Writes that no
        counter sees (`p.data.copy_`, collectives, raw pointers) need an explicit policy_dirty()"""
        v = sum(p._version for p in params) + self.online._version
        if v != getattr(self, "_param_versions", None):
            self._param_versions = v
            self.policy_dirty()

    def act_sample(self, obs, eps):
        """dsact_act_sample: (action float32[A], logp float) of TanhGaussDistribution.sample() for ONE observation with the
        caller's N(0,1) draw eps[A]; obs / eps are contiguous float32 arrays (no copies are made here)"""
        if getattr(self, "_act_out", None) is None:
            self._act_out = np.empty(self.act_dim, np.float32)
            self._act_lp = np.empty(1, np.float32)
            self._act_out_p, self._act_lp_p = _ffi.fptr(self._act_out), _ffi.fptr(self._act_lp)
        rc = self._lib.dsact_act_sample(self._h, obs.ctypes.data_as(_ffi._FP), eps.ctypes.data_as(_ffi._FP),
                                        self._act_out_p, self._act_lp_p)
        if rc != 0:
            self._chk(rc)
        return self._act_out, self._act_lp

    def _addr_fn(self, attr: str, symbol: str, argtypes):
        """a second binding of `symbol` whose pointer arguments are void* (plain integer addresses cross without a ctypes pointer
        object per call), cached as self.<attr> by the first call"""
        f = self._lib[symbol]          # a fresh function object: its argtypes are its own
        f.restype, f.argtypes = C.c_int, argtypes
        setattr(self, attr, f)
        return f

    def act_sample_addr(self, obs_addr: int, eps_addr: int, act_addr: int, logp_addr: int):
        """dsact_act_sample on plain integer addresses (the sampler's per-step call: no array or pointer objects are made;
        results land in the caller's rows). A second binding of the same symbol whose arguments are void*."""
        f = getattr(self, "_act_addr_fn", None) or self._addr_fn("_act_addr_fn", "dsact_act_sample", [C.c_void_p] * 5)
        rc = f(self._h, obs_addr, eps_addr, act_addr, logp_addr)
        if rc != 0:
            self._chk(rc)

    def act_sample_batch(self, obs, eps):
        """dsact_act_sample_batch: (action float32[N, A], logp float32[N]) of the policy's action distribution sampled for N
        observation rows with the caller's N(0,1) draws eps[N, A] (row i: torch.randn(N, A)[i]). obs / eps: numpy / CPU
        tensors, or CUDA tensors on this engine's GPU (passed by device address, as load_batch does). A CNN engine with
        cnn_act takes frames as [N, C, H, W] or [N, O] rows (O = C * H * W)"""
        torch = self.torch
        n = int(np.prod(np.shape(obs))) // self.obs_dim
        srcs = [self._src(obs, n * self.obs_dim), self._src(eps, n * self.act_dim)]
        if any(isinstance(k, torch.Tensor) for _, k in srcs):
            torch.cuda.current_stream(self.device).synchronize()   # the producers of the CUDA sources have finished
        act = np.empty((n, self.act_dim), np.float32)
        lp = np.empty(n, np.float32)
        self._chk(self._lib.dsact_act_sample_batch(self._h, srcs[0][0], n, srcs[1][0], _ffi.fptr(act), _ffi.fptr(lp)))
        return act, lp

    def act_sample_batch_addr(self, obs_addr: int, n: int, eps_addr: int, act_addr: int, logp_addr: int):
        """dsact_act_sample_batch on plain integer addresses (the vectorised sampler's per-step call; results land in the
        caller's rows). A second binding of the same symbol whose pointer arguments are void*."""
        f = getattr(self, "_act_batch_addr_fn", None) or self._addr_fn(
            "_act_batch_addr_fn", "dsact_act_sample_batch", [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p])
        rc = f(self._h, obs_addr, n, eps_addr, act_addr, logp_addr)
        if rc != 0:
            self._chk(rc)

    def act_mode_batch(self, obs) -> np.ndarray:
        """dsact_act_mode_batch: action float32[N, A], the action distribution's mode() of policy(obs) for N observation rows
        (the evaluator's deterministic acting). obs: numpy / CPU tensors, or (MLP policies) CUDA tensors on this engine's GPU.
        Callers that may have written the policy with torch ops call note_torch_writes(policy.parameters()) first."""
        torch = self.torch
        n = int(np.prod(np.shape(obs))) // self.obs_dim
        if self.conv_type and isinstance(obs, torch.Tensor):
            obs = obs.detach().cpu()   # (the CNN route reads host frames)
        src = self._src(obs, n * self.obs_dim)
        if isinstance(src[1], torch.Tensor):
            torch.cuda.current_stream(self.device).synchronize()   # the producer of the CUDA source has finished
        act = np.empty((n, self.act_dim), np.float32)
        self._chk(self._lib.dsact_act_mode_batch(self._h, src[0], n, _ffi.fptr(act)))
        return act

    def act_mode_batch_addr(self, obs_addr: int, n: int, act_addr: int):
        """dsact_act_mode_batch on plain integer addresses (the vectorised evaluator's per-step call; the actions land in the
        caller's rows). A second binding of the same symbol whose pointer arguments are void*."""
        f = getattr(self, "_act_mode_addr_fn", None) or self._addr_fn(
            "_act_mode_addr_fn", "dsact_act_mode_batch", [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])
        rc = f(self._h, obs_addr, n, act_addr)
        if rc != 0:
            self._chk(rc)

    # ---- device-resident sampling: everything stays on the GPU, nothing waits -------------------------
    @staticmethod
    def _rows(t) -> int:
        """the leading dimension of a tensor argument (0 for anything else: _dev then refuses it by name)"""
        return int(t.shape[0]) if hasattr(t, "shape") and len(t.shape) else 0

    def _dev(self, t, shape, dtypes, name):
        """address of a torch tensor the asynchronous entry points may read or write: on this engine's GPU, contiguous, of
        the given shape and one of `dtypes`"""
        torch = self.torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != self.device_index:
            raise ValueError("%s must be a torch tensor on %s (got %s)" % (name, self.device, getattr(t, "device", type(t).__name__)))
        if t.dtype not in dtypes:
            raise ValueError("%s must have dtype %s (got %s)" % (name, " or ".join(str(d) for d in dtypes), t.dtype))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
        if tuple(t.shape) != tuple(shape):
            raise ValueError("%s must have shape %r (got %r)" % (name, tuple(shape), tuple(t.shape)))
        return t.data_ptr()

    def set_act_rng(self, seed: int):
        """dsact_set_act_rng: Philox key of act_sample_device's in-kernel N(0,1) draw; 0 switches it off (the default)"""
        self._chk(self._lib.dsact_set_act_rng(self._h, int(seed)))
        self.act_seed = int(seed)

    def set_explore_noise(self, mean=None, std=None):
        """dsact_set_explore_noise: GaussNoise(mean, std) added to act_sample_device's sampled action before the clip, drawn in
        the kernel on Philox stream 6 (needs set_act_rng). None: off (the default). Scalars or one-element arrays: ONE normal per
        (row, step) for every action dimension; arrays of length act_dim: one per dimension. The host-returning calls, the
        mode calls and the evaluators are not affected."""
        if mean is None and std is None:
            self._chk(self._lib.dsact_set_explore_noise(self._h, None, None, 0))
            return
        if mean is None or std is None:
            raise ValueError("set_explore_noise takes mean and std together (or neither: off)")
        m, s = np.broadcast_arrays(_f32(mean).reshape(-1), _f32(std).reshape(-1))
        m, s = np.ascontiguousarray(m), np.ascontiguousarray(s)
        self._chk(self._lib.dsact_set_explore_noise(self._h, _ffi.fptr(m), _ffi.fptr(s), int(m.shape[0])))

    def act_sample_device(self, obs, eps, step, action, clipped, logp):
        """dsact_act_sample_device: policy(obs[n, O]) on the live weights + the action distribution's sample, written into the
        caller's device tensors action[n, A] (what the ring stores), clipped[n, A] (inside the action limits: what the
        environment receives) and logp[n]. eps[n, A]: the caller's N(0,1) draws, or None: drawn in the kernel for acting step
        `step` (set_act_rng). float32 contiguous tensors on this engine's GPU. Asynchronous on the engine's stream: issue the
        torch work that produces obs / consumes the results under `torch.cuda.stream(engine.torch_stream)`."""
        f32 = (self.torch.float32,)
        n = self._rows(obs)
        O, A = self.obs_dim, self.act_dim
        po, u8 = self._frames(obs, n, "obs")
        pe = self._dev(eps, (n, A), f32, "eps") if eps is not None else None
        pa, pc, pl = self._dev(action, (n, A), f32, "action"), self._dev(clipped, (n, A), f32, "clipped"), self._dev(logp, (n,), f32, "logp")
        fn = self._lib.dsact_act_sample_device_u8 if u8 else self._lib.dsact_act_sample_device
        rc = fn(self._h, po, n, pe, int(step), pa, pc, pl)
        if rc != 0:
            self._chk(rc)

    # ---- a sample() as one captured graph: the acting step lives in device memory --------------------------
    def act_counter_set(self, step: int):
        """dsact_act_counter_set: the acting-step counter's device word = step (mod 2^64), written in stream order. Refused under
        stream capture (the value would be baked into the graph)."""
        self._chk(self._lib.dsact_act_counter_set(self._h, int(step) & 0xFFFFFFFFFFFFFFFF))

    def act_counter_add(self, k: int):
        """dsact_act_counter_add: counter += k in stream order. Legal under stream capture: the node that closes a captured
        sample()."""
        rc = self._lib.dsact_act_counter_add(self._h, int(k))
        if rc != 0:
            self._chk(rc)

    def act_counter_read(self) -> int:
        """dsact_act_counter_read: the counter behind everything enqueued so far. WAITS for the engine's stream."""
        v = C.c_uint64()
        self._chk(self._lib.dsact_act_counter_read(self._h, C.byref(v)))
        return int(v.value)

    def act_sample_device_counted(self, obs, step_offset, action, clipped, logp):
        """dsact_act_sample_device_counted: act_sample_device(obs, None, counter + step_offset, ...) with the counter read on the
        device when the launch runs (act_counter_set first) -- bit for bit that call's action[n, A], clipped[n, A] and logp[n].
        MLP policies, obs[n, O] float32; a CNN engine after cnn_acting_capture: frames as act_sample_device takes them, float32
        or uint8 (the call dispatches on the dtype). Asynchronous, and legal while the engine's stream is being captured into a
        graph (after one call outside the capture, which makes the library's allocations)."""
        f32 = (self.torch.float32,)
        n = self._rows(obs)
        A = self.act_dim
        po, u8 = self._frames(obs, n, "obs")
        pa, pc, pl = self._dev(action, (n, A), f32, "action"), self._dev(clipped, (n, A), f32, "clipped"), self._dev(logp, (n,), f32, "logp")
        fn = self._lib.dsact_act_sample_device_counted_u8 if u8 else self._lib.dsact_act_sample_device_counted
        rc = fn(self._h, po, n, int(step_offset), pa, pc, pl)
        if rc != 0:
            self._chk(rc)

    def step_frames_device(self, obs2, rew, terminated, truncated, obs2_slot, rew_slot, terminated_slot, truncated_slot, ended):
        """dsact_step_frames_device: step_rows_device for image rows -- obs2[n, C, H, W] (or any [n, ...] rows) uint8 or float32
        -> obs2_slot of the same shape and dtype, a row split over several workgroups; the scalar columns and ended as there.
        Contiguous tensors on this engine's GPU. Asynchronous; legal under stream capture."""
        torch = self.torch
        f32, flag, img = (torch.float32,), (torch.bool, torch.uint8), (torch.float32, torch.uint8)
        n = self._rows(rew)
        shape = tuple(obs2.shape) if hasattr(obs2, "shape") else ()
        if len(shape) < 2 or shape[0] != n or getattr(obs2_slot, "dtype", None) != obs2.dtype:
            raise ValueError("obs2 must be [n, ...] rows with n = %d and obs2_slot of its dtype (got %r, %s and %s)"
                             % (n, shape, getattr(obs2, "dtype", None), getattr(obs2_slot, "dtype", None)))
        ptrs = [self._dev(obs2, shape, img, "obs2"), self._dev(rew, (n,), f32, "rew"),
                self._dev(terminated, (n,), flag, "terminated"), self._dev(truncated, (n,), flag, "truncated"),
                self._dev(obs2_slot, shape, img, "obs2_slot"), self._dev(rew_slot, (n,), f32, "rew_slot"),
                self._dev(terminated_slot, (n,), flag, "terminated_slot"), self._dev(truncated_slot, (n,), flag, "truncated_slot"),
                self._dev(ended, (n,), flag, "ended")]
        row_bytes = int(obs2[0].numel()) * int(obs2.element_size())
        rc = self._lib.dsact_step_frames_device(self._h, n, row_bytes, *ptrs)
        if rc != 0:
            self._chk(rc)

    def step_rows_device(self, obs2, rew, terminated, truncated, obs2_slot, rew_slot, terminated_slot, truncated_slot, ended):
        """dsact_step_rows_device: one lockstep step's row copies in one launch -- obs2[n, W] -> obs2_slot, rew[n] -> rew_slot,
        terminated / truncated [n] -> their slots (the slots: n-row slices of the [S, .] sample buffers), and ended[n] =
        terminated | truncated. float32 / bool (or uint8) contiguous tensors on this engine's GPU. Asynchronous; legal under
        stream capture."""
        torch = self.torch
        f32, flag = (torch.float32,), (torch.bool, torch.uint8)
        n = self._rows(rew)
        W = int(obs2.shape[1]) if hasattr(obs2, "shape") and len(obs2.shape) == 2 else 0
        ptrs = [self._dev(obs2, (n, W), f32, "obs2"), self._dev(rew, (n,), f32, "rew"),
                self._dev(terminated, (n,), flag, "terminated"), self._dev(truncated, (n,), flag, "truncated"),
                self._dev(obs2_slot, (n, W), f32, "obs2_slot"), self._dev(rew_slot, (n,), f32, "rew_slot"),
                self._dev(terminated_slot, (n,), flag, "terminated_slot"), self._dev(truncated_slot, (n,), flag, "truncated_slot"),
                self._dev(ended, (n,), flag, "ended")]
        rc = self._lib.dsact_step_rows_device(self._h, n, W, *ptrs)
        if rc != 0:
            self._chk(rc)

    def env_wrap_step(self, n, obs2=None, rew=None, terminated=None, truncated=None, obs_shift=None, obs_scale=None,
                      reward_shift=0.0, reward_scale=1.0, reward_on=False, max_episode_steps=0, elapsed=None, obs2_out=None,
                      rew_out=None, truncated_out=None):
        """dsact_env_wrap_step: the reference's environment wrappers behind a tensor environment's step in one launch (DESIGN.md
        section 27). A part is on when its output is given: obs2_out[n, ...] = (obs2 + obs_shift) * obs_scale (float32 rows of
        any shape, obs_shift / obs_scale one flat row), rew_out[n] = (rew + reward_shift) * reward_scale (reward_on),
        truncated_out[n] = truncated | (elapsed >= M & ~terminated) after elapsed = min(elapsed + 1, M) (int32 [n], M =
        max_episode_steps > 0). Contiguous tensors on this engine's GPU; an output may be its input. Asynchronous; legal under
        stream capture."""
        torch = self.torch
        f32, flag, i32 = (torch.float32,), (torch.bool, torch.uint8), (torch.int32,)
        n, W, M = int(n), 0, int(max_episode_steps)
        po = ps = pc = pr = pt = pu = pe = poo = pro = puo = None
        if obs2_out is not None:
            shape = tuple(obs2.shape) if hasattr(obs2, "shape") else ()
            W = int(obs2[0].numel()) if len(shape) >= 2 and shape[0] == n else 0
            po, poo = self._dev(obs2, shape, f32, "obs2"), self._dev(obs2_out, shape, f32, "obs2_out")
            ps, pc = self._dev(obs_shift, (W,), f32, "obs_shift"), self._dev(obs_scale, (W,), f32, "obs_scale")
        if reward_on:
            pr, pro = self._dev(rew, (n,), f32, "rew"), self._dev(rew_out, (n,), f32, "rew_out")
        if M > 0:
            pt, pu = self._dev(terminated, (n,), flag, "terminated"), self._dev(truncated, (n,), flag, "truncated")
            pe, puo = self._dev(elapsed, (n,), i32, "elapsed"), self._dev(truncated_out, (n,), flag, "truncated_out")
        rc = self._lib.dsact_env_wrap_step(self._h, n, W, po, pr, pt, pu, ps, pc, float(reward_shift), float(reward_scale),
                                           1 if reward_on else 0, M, pe, poo, pro, puo)
        if rc != 0:
            self._chk(rc)

    def env_wrap_reset(self, n, obs=None, mask=None, obs_shift=None, obs_scale=None, elapsed=None, obs_out=None):
        """dsact_env_wrap_reset: the wrappers behind a tensor environment's reset in one launch -- obs_out[n, ...] = (obs +
        obs_shift) * obs_scale for EVERY row (on when obs_out is given) and elapsed[i] = 0 where the bool / uint8 mask[n] is set
        (mask None: every row; on when elapsed is given). Contiguous tensors on this engine's GPU. Asynchronous; legal under
        stream capture."""
        torch = self.torch
        f32, flag, i32 = (torch.float32,), (torch.bool, torch.uint8), (torch.int32,)
        n, W = int(n), 0
        po = ps = pc = poo = pe = pm = None
        if obs_out is not None:
            shape = tuple(obs.shape) if hasattr(obs, "shape") else ()
            W = int(obs[0].numel()) if len(shape) >= 2 and shape[0] == n else 0
            po, poo = self._dev(obs, shape, f32, "obs"), self._dev(obs_out, shape, f32, "obs_out")
            ps, pc = self._dev(obs_shift, (W,), f32, "obs_shift"), self._dev(obs_scale, (W,), f32, "obs_scale")
        if elapsed is not None:
            pe = self._dev(elapsed, (n,), i32, "elapsed")
            pm = None if mask is None else self._dev(mask, (n,), flag, "mask")
        rc = self._lib.dsact_env_wrap_reset(self._h, n, W, po, pm, ps, pc, pe, poo)
        if rc != 0:
            self._chk(rc)

    def _frame_pipe_rows(self, n, raw, stack, out, frame_stack, gray, out_name):
        """(slot_elems, gray flag, elem_size, the three addresses) of a frame-pipe call: raw[n, ...] uint8 or float32 (with gray
        [n, 3, H, W] for "chw", [n, H, W, 3] for "hwc"), stack / out [n, frame_stack * slot] of the slot's dtype"""
        torch = self.torch
        n, K = int(n), int(frame_stack)
        flag = {None: 0, "chw": 1, "hwc": 2}.get(gray, -1)
        shape = tuple(raw.shape) if hasattr(raw, "shape") else ()
        pr = self._dev(raw, shape, (torch.uint8, torch.float32), "raw")
        if len(shape) < 2 or shape[0] != n:
            raise ValueError("raw must have shape [%d, ...] (got %r)" % (n, shape))
        elems = int(raw[0].numel())
        if flag > 0:
            if len(shape) != 4 or shape[1 if flag == 1 else 3] != 3:
                raise ValueError("raw must be 3-channel %s frames (got %r)" % (gray, shape))
            elems //= 3
        odt = (torch.float32,) if flag > 0 else (raw.dtype,)
        want = (n, max(K, 0) * elems)
        ps = self._dev(stack.view(n, -1) if hasattr(stack, "view") else stack, want, odt, "stack")
        po = self._dev(out.view(n, -1) if hasattr(out, "view") else out, want, odt, out_name)
        return elems, flag, int(raw.element_size()), pr, ps, po

    def frame_pipe_step(self, n, j, action_repeat, frame_stack, gray, raw, rew, terminated, truncated, stack, acc, ended_at, flags,
                        obs2_out, rew_out, terminated_out, truncated_out):
        """dsact_frame_pipe_step: launch j of action_repeat of the reference's image pipeline behind a tensor environment's inner
        step -- gray (None, "chw", "hwc") of raw[n, ...], the stack[n, frame_stack * slot] shifted at
        j == 0 and its newest slot overwritten while the row is alive, the reward summed into acc[n], the ending step's flags
        kept in flags[n] / ended_at[n] (int32), and at j == action_repeat - 1 the four outputs written. Contiguous tensors on
        this engine's GPU. Asynchronous; legal under stream capture."""
        torch = self.torch
        f32, flag, i32 = (torch.float32,), (torch.bool, torch.uint8), (torch.int32,)
        n = int(n)
        elems, g, esize, pr, ps, po = self._frame_pipe_rows(n, raw, stack, obs2_out, frame_stack, gray, "obs2_out")
        rc = self._lib.dsact_frame_pipe_step(
            self._h, n, elems, int(frame_stack), int(action_repeat), int(j), g, esize, pr, self._dev(rew, (n,), f32, "rew"),
            self._dev(terminated, (n,), flag, "terminated"), self._dev(truncated, (n,), flag, "truncated"), ps,
            self._dev(acc, (n,), f32, "acc"), self._dev(ended_at, (n,), i32, "ended_at"), self._dev(flags, (n,), (torch.uint8,), "flags"),
            po, self._dev(rew_out, (n,), f32, "rew_out"), self._dev(terminated_out, (n,), flag, "terminated_out"),
            self._dev(truncated_out, (n,), flag, "truncated_out"))
        if rc != 0:
            self._chk(rc)

    def frame_pipe_reset(self, n, frame_stack, gray, raw, mask, stack, obs_out):
        """dsact_frame_pipe_reset: rows whose bool / uint8 mask[n] is set (None: every row) fill all frame_stack slots of
        stack[n, frame_stack * slot] from (the gray of) raw[n, ...]; every row's stack is then copied to obs_out. Contiguous
        tensors on this engine's GPU. Asynchronous; legal under stream capture."""
        torch = self.torch
        n = int(n)
        elems, g, esize, pr, ps, po = self._frame_pipe_rows(n, raw, stack, obs_out, frame_stack, gray, "obs_out")
        pm = None if mask is None else self._dev(mask, (n,), (torch.bool, torch.uint8), "mask")
        rc = self._lib.dsact_frame_pipe_reset(self._h, n, elems, int(frame_stack), g, esize, pr, pm, ps, po)
        if rc != 0:
            self._chk(rc)

    def _frames(self, t, n, name):
        """(address, is_uint8) of the observation rows of a device-resident call: [n, O] float32, and on a CNN engine with cnn_act
         also [n, C, H, W] rows and uint8 tensors of either shape -- byte frames, codes into the coded
        ring's codebook (the library refuses them on any other handle)"""
        torch = self.torch
        O = self.obs_dim
        shape, dtypes = (n, O), (torch.float32,)
        if self.conv_type and self.cnn_act:
            dtypes = (torch.float32, torch.uint8)
            if hasattr(t, "shape") and len(t.shape) == 4:
                shape = (n,) + tuple(self.obs_shape)
        return self._dev(t, shape, dtypes, name), getattr(t, "dtype", None) == torch.uint8

    def buffer_add_device(self, obs, act, rew, obs2, terminated, truncated, logp, reward_scale=1.0):
        """dsact_buffer_add_device: n transitions from device tensors into ring rows (ptr + i) % capacity; rew is stored as
        rew * reward_scale, done as terminated & ~truncated. obs / obs2 [n, O], act [n, A], rew / logp [n] float32,
        terminated / truncated [n] bool (or uint8). Asynchronous on the engine's stream. A CNN engine with cnn_act takes image
        rows as [n, O] or [n, C, H, W], float32 or -- with a coded ring -- uint8 codes (obs and obs2 in the same dtype)."""
        torch = self.torch
        f32, flag = (torch.float32,), (torch.bool, torch.uint8)
        n = self._rows(rew)
        A = self.act_dim
        (po, u8), (po2, u8_2) = self._frames(obs, n, "obs"), self._frames(obs2, n, "obs2")
        if u8 != u8_2:
            raise ValueError("obs and obs2 must have the same dtype (got %s and %s)" % (obs.dtype, obs2.dtype))
        ptrs = [po, self._dev(act, (n, A), f32, "act"), self._dev(rew, (n,), f32, "rew"),
                po2, self._dev(terminated, (n,), flag, "terminated"),
                self._dev(truncated, (n,), flag, "truncated"), self._dev(logp, (n,), f32, "logp")]
        fn = self._lib.dsact_buffer_add_device_u8 if u8 else self._lib.dsact_buffer_add_device
        self._chk(fn(self._h, n, *ptrs, float(reward_scale)))
        self.rows_added += n

    # ---- device-resident evaluation: launches only, one wait in eval_poll ------------------------------
    def act_mode_device(self, obs, action):
        """dsact_act_mode_device: the action distribution's mode() of policy(obs[n, O]) on the live weights, written into the
        caller's device tensor action[n, A] (bit for bit act_mode_batch's GPU route). float32 contiguous tensors on this engine's
        GPU. Asynchronous on the engine's stream: issue the torch work that produces obs / consumes action under
        `torch.cuda.stream(engine.torch_stream)`."""
        f32 = (self.torch.float32,)
        n = self._rows(obs)
        (po, u8), pa = self._frames(obs, n, "obs"), self._dev(action, (n, self.act_dim), f32, "action")
        rc = (self._lib.dsact_act_mode_device_u8 if u8 else self._lib.dsact_act_mode_device)(self._h, po, n, pa)
        if rc != 0:
            self._chk(rc)

    def eval_begin(self, n_envs: int, n_episodes: int):
        """dsact_eval_begin: the episode bookkeeping for n_envs lockstep rows and n_episodes episodes, initialised in stream
        order (row i plays episode i, then i + n_envs, ...)"""
        self._chk(self._lib.dsact_eval_begin(self._h, int(n_envs), int(n_episodes)))
        self._eval_n = int(n_envs)

    def eval_commit(self, reward, terminated, truncated, ended):
        """dsact_eval_commit: one lockstep step of the bookkeeping. reward[N] float32, terminated / truncated [N] bool (or uint8)
        in; ended[N] bool (or uint8) out = terminated | truncated, the mask for env.reset. Asynchronous on the engine's stream."""
        torch = self.torch
        f32, flag = (torch.float32,), (torch.bool, torch.uint8)
        n = getattr(self, "_eval_n", None)
        if n is None:
            n = self._rows(reward)   # (the library refuses: E_STATE)
        ptrs = [self._dev(reward, (n,), f32, "reward"), self._dev(terminated, (n,), flag, "terminated"),
                self._dev(truncated, (n,), flag, "truncated"), self._dev(ended, (n,), flag, "ended")]
        rc = self._lib.dsact_eval_commit(self._h, *ptrs)
        if rc != 0:
            self._chk(rc)

    def eval_poll(self) -> int:
        """dsact_eval_poll: the number of episodes that have not ended, behind everything enqueued so far. WAITS for the
        engine's stream: the one wait of an evaluation loop."""
        v = C.c_int32()
        self._chk(self._lib.dsact_eval_poll(self._h, C.byref(v)))
        return int(v.value)

    def eval_read(self, n_episodes: int):
        """dsact_eval_read: (returns float64[E], lengths int32[E]) in episode-index order, once every episode has ended
        (DsactError E_STATE before that)"""
        E = int(n_episodes)
        returns, lengths = np.empty(max(E, 0), np.float64), np.empty(max(E, 0), np.int32)
        self._chk(self._lib.dsact_eval_read(self._h, returns.ctypes.data_as(C.c_void_p), lengths.ctypes.data_as(C.c_void_p), E))
        return returns, lengths

    # ---- the evaluation trace: eval_save's lists of the first episodes, kept on the device ----------------
    def eval_trace_begin(self, n_saved: int, max_steps: int, obs_row_bytes: int):
        """dsact_eval_trace_begin (after eval_begin): record the first n_saved episodes of the running evaluation, up to max_steps
        steps each; obs_row_bytes is one observation row in bytes (4 * obs_dim; image engines: C*H*W bytes of uint8 frames or
        4*C*H*W of float32 frames). Allocates on growth only (eval_state_gen then goes up)."""
        self._chk(self._lib.dsact_eval_trace_begin(self._h, int(n_saved), int(max_steps), int(obs_row_bytes)))
        self._trace_row_bytes = int(obs_row_bytes)

    def eval_trace_end(self):
        """dsact_eval_trace_end: the trace goes inactive (its arrays are kept for the next eval_trace_begin)"""
        self._chk(self._lib.dsact_eval_trace_end(self._h))

    def eval_record(self, obs, action):
        """dsact_eval_record: one lockstep step of the trace, BEFORE the environment steps -- obs[N, O] float32 (image engines:
        frames as act_mode_device takes them, float32 or uint8) and action[N, A] float32, the action the environment receives.
        Contiguous tensors on this engine's GPU. Asynchronous; legal under stream capture."""
        n = getattr(self, "_eval_n", None)
        if n is None:
            n = self._rows(obs)   # (the library refuses: E_STATE)
        (po, _), pa = self._frames(obs, n, "obs"), self._dev(action, (n, self.act_dim), (self.torch.float32,), "action")
        rc = self._lib.dsact_eval_record(self._h, po, pa)
        if rc != 0:
            self._chk(rc)

    def eval_trace_read(self, episode: int, capacity_rows: int):
        """dsact_eval_trace_read: (obs uint8[rows, obs_row_bytes] -- the raw bytes of the rows --, act float32[rows, A], rew
        float32[rows]) of one saved episode, rows = min(its length, max_steps) <= capacity_rows. WAITS; DsactError E_STATE while
        an episode has not ended."""
        cap = max(int(capacity_rows), 0)
        rb = getattr(self, "_trace_row_bytes", 4 * self.obs_dim)
        obs, act, rew = np.empty((cap, rb), np.uint8), np.empty((cap, self.act_dim), np.float32), np.empty(cap, np.float32)
        rows = C.c_int32()
        self._chk(self._lib.dsact_eval_trace_read(self._h, int(episode), obs.ctypes.data_as(C.c_void_p), act.ctypes.data_as(C.c_void_p),
                                                  rew.ctypes.data_as(C.c_void_p), cap, C.byref(rows)))
        n = int(rows.value)
        return obs[:n], act[:n], rew[:n]

    # ---- episode statistics of the training environments: one launch per commit, one wait in track_read ---
    TRACK_COLUMNS = (("episodes", np.int64), ("terminated", np.int64), ("ret_sum", np.float64), ("ret_min", np.float64),
                     ("ret_max", np.float64), ("len_sum", np.int64), ("last_ret", np.float64), ("last_len", np.int32),
                     ("cur_ret", np.float64), ("cur_len", np.int32))     # dsact_track_read's arrays, in its argument order

    def track_begin(self, n_envs: int):
        """dsact_track_begin: new episode statistics for n_envs lockstep rows, initialised in stream order"""
        self._chk(self._lib.dsact_track_begin(self._h, int(n_envs)))
        self._track_n = int(n_envs)

    def track_commit(self, reward, terminated, truncated, n_steps: int):
        """dsact_track_commit: n_steps lockstep steps of the bookkeeping in one launch. reward[n_steps * N] float32 (before any
        reward scale), terminated / truncated [n_steps * N] bool (or uint8), step-major. Asynchronous on the engine's stream."""
        torch = self.torch
        f32, flag = (torch.float32,), (torch.bool, torch.uint8)
        T = int(n_steps)
        n = getattr(self, "_track_n", None)
        rows = T * n if n is not None and T > 0 else self._rows(reward)   # (the library refuses: E_STATE / E_INVALID)
        ptrs = [self._dev(reward, (rows,), f32, "reward"), self._dev(terminated, (rows,), flag, "terminated"),
                self._dev(truncated, (rows,), flag, "truncated")]
        rc = self._lib.dsact_track_commit(self._h, *ptrs, T)
        if rc != 0:
            self._chk(rc)

    def track_read(self, clear: bool = True) -> dict:
        """dsact_track_read: {name: array[N]} of TRACK_COLUMNS behind everything enqueued so far. WAITS for the engine's stream.
        clear: the totals start again afterwards (the episodes in progress, cur_ret / cur_len, go on)."""
        n = getattr(self, "_track_n", None) or 0
        out = {k: np.empty(max(n, 1), dt) for k, dt in self.TRACK_COLUMNS}   # (n = 0: the library refuses, E_STATE)
        self._chk(self._lib.dsact_track_read(self._h, n, *[a.ctypes.data_as(C.c_void_p) for a in out.values()], 1 if clear else 0))
        return {k: a[:n] for k, a in out.items()}

    def behaviour_hold(self):
        """dsact_behaviour_hold: from now on act_sample / act_sample_batch act with a copy of the policy taken on the engine's
        stream behind everything enqueued so far -- without waiting for anything enqueued later (act_mode_batch and
        policy_forward stay live). MLP policies only; refused under stream capture."""
        self._chk(self._lib.dsact_behaviour_hold(self._h))

    def behaviour_release(self):
        """dsact_behaviour_release: act_sample / act_sample_batch act with the live weights again"""
        self._chk(self._lib.dsact_behaviour_release(self._h))

    def stream_idle(self) -> bool:
        """dsact_stream_idle: True when everything enqueued on the engine's stream has completed (never blocks)"""
        rc = self._lib.dsact_stream_idle(self._h)
        if rc < 0:
            self._chk(rc)
        return rc == 1

    def policy_forward(self, obs) -> np.ndarray:
        obs = _f32(obs).reshape(-1, self.obs_dim)
        n = obs.shape[0]
        out = np.empty((n, 2 * self.act_dim), np.float32)
        for s in range(0, n, 64):
            e = min(n, s + 64)
            chunk = np.ascontiguousarray(obs[s:e])
            o = np.empty((e - s, 2 * self.act_dim), np.float32)
            self._chk(self._lib.dsact_policy_forward(self._h, _ffi.fptr(chunk), e - s, _ffi.fptr(o)))
            out[s:e] = o
        return out


# process-wide registry: the replay buffer plugin shares the algorithm's handle so that a gathered
# minibatch never leaves HBM (mix-and-match case iii)
_CURRENT = None


def register_engine(engine: "DsactEngine"):
    global _CURRENT
    _CURRENT = engine


def current_engine() -> Optional["DsactEngine"]:
    return _CURRENT
