"""frame_pipe_tensor_env -- the reference's image pipeline (env_gym/gym_carracing_data.py:23-69: rgb2gray, the stack of the last
img_stack frames, action_repeat simulator steps per action; gym_breakout_data.py's FrameStack(4) / frame_skip=4 and
gym_cartpolecontiwithstack_data.py's stacked vectors are the same rules) for BATCHED TENSOR ENVIRONMENTS, one launch behind
every inner step and one behind a reset.

`frame_pipe_tensor_env(env, gray=None, frame_stack=None, action_repeat=None)` takes an environment that speaks the
tensor-environment protocol of training/hip_tensor_sampler.py and returns a FramePipeTensorEnv that speaks it too, so sampler,
evaluator, captured graphs, eval_save, episode statistics and run states work with it unchanged. With every argument None it
returns `env` itself.

The rules are the reference's (gym_carracing_data.py:23-69):
  gray    gray="chw" / "hwc": the inner environment returns RAW pixel values as [N, 3, H, W] / [N, H, W, 3] rows, uint8 (values
          0..255, not codes) or float32. A frame becomes ONE float32 plane [N, 1, H, W],
              out = float32( ((R*0.299 + G*0.587) + B*0.114) / 128.0 - 1.0 )
          in float64 (0.299, 0.587, 0.114 the float64 literals), every multiply and add rounded on its own and never contracted
          into an FMA. (np.dot's summation order in the reference depends on the BLAS route it takes for the array's shape, so
          the reference's float64 value is not one fixed bit pattern: this rule and the reference differ by at most one float32
          step, in 1-2 elements per million.) Without gray a row passes through in its own dtype -- uint8 rows are then codes
          and stay uint8, stacking only copies -- and may be of any shape, [N, C, H, W] frames or [N, O] vectors: a row is a
          flat run of elements.
  stack   frame_stack=K >= 1 (<= 64): the observation is the last K (gray or passed-through) rows, oldest first, newest last:
          [N, K, H, W] with gray, [N, K*C, H, W] without, [N, K*O] for vector rows. reset() and every row restarted by
          reset(mask) get K copies of the row's reset frame; untouched rows keep their stack. frame_stack=None is K = 1.
  repeat  action_repeat=R >= 1: one outer step(action) makes exactly R inner env.step(action) calls with the same action tensor,
          no inner reset and no host decision, so a graph holds all R. Per row: it is ALIVE until an inner step returns
          terminated | truncated for it; the reward is the float32 sum of the live inner steps' rewards in order (acc = r_0,
          then acc = acc + r_j, one rounded add each -- NumPy 2 keeps the reference's `0 + np.float32` in float32);
          terminated / truncated are the inner flags of the step at which the row ended, both False if it did not end; the
          frame pushed onto the stack is the one of the row's LAST LIVE inner step -- one outer step pushes one frame. Inner
          steps after a row has ended are ignored for that row, but the inner environment IS still stepped for it: A TENSOR
          ENVIRONMENT UNDER action_repeat MUST TOLERATE BEING STEPPED ON AN ENDED ROW; the wrapper's reset(mask) restarts it
          afterwards. `ended_at` (int32 [N]) holds the inner index at which a row ended in the last outer step, -1 if it did not.
The CarRacing-specific parts of the reference's Env -- the `a[0] * 2 - 1` action map and the 100-step reward memory -- are the
environment's business and stay out.

Buffers, allocated once at the first reset() (when a row's shape, dtype and device are known): the private stack state `stack`,
step's obs2 and reset's obs -- three buffers of one stacked row each per environment. step's obs2 is the true next observation
and survives the following reset(mask); reset's return survives the following step: the sampler copies in stream order and the
tensor evaluator reads in place under hip_graph_eval. Reward and flag outputs are wrapper-owned too.

Forwarded: `capture_safe` is the inner environment's value (the wrapper itself keeps the promise: in-place state, no allocation
that outlives a call, nothing on the host, torch's current stream); `num_envs`, `action_low`, `action_high` and every other
attribute forward to the inner environment. Own: `obs_shape` (the stacked row's shape; before the first reset() from the inner
environment's `obs_shape` / `obs_dim` where it names one), `obs_dim` (its length), `frame_stack`, `action_repeat`.

Two routes, bit for bit equal:
  torch route  in-place / out= torch ops only, a dozen small launches per inner step. CPU and GPU; the restatement the tests
               compare against (float64 `mul` / `add` ops, one each, for the gray).
  fused route  dsact_frame_pipe_step / dsact_frame_pipe_reset (k_frame_pipe_step / k_frame_pipe_reset, csrc/dsact_kernels.h): ONE
               launch behind each inner step and ONE behind a reset. Selected by `bind_engine(engine)` with a DsactEngine on the
               tensors' GPU; `fused` tells which route is active. The launches go to the engine's stream, so a bound wrapper is
               stepped and reset under `torch.cuda.stream(engine.torch_stream)` (anything else is a RuntimeError). On the fused
               route a tensor the inner environment returns in another dtype or on another device is a TypeError, never a quiet
               change of route. `use_fused = False` on an instance keeps the torch route whatever is bound.

Run state: state_dict() -> {"format", "params", "stack" (CPU), "inner": env.state_dict()}; an inner environment without the
method raises require_env_state's NotImplementedError. load_state_dict refuses other parameters or another stack shape / dtype
(ValueError) and copies the stack into place. The per-call scratch (reward accumulator, ended marker) is not state.

Refused by frame_pipe_tensor_env before any environment call (ValueError): gray not in {None, "chw", "hwc"}; a non-integer, bool
or < 1 frame_stack / action_repeat; frame_stack > 64. At the first reset(): with gray, rows that are not 3-channel in the named
layout (ValueError) or neither uint8 nor float32 (TypeError).

Composition: the pipeline sits INSIDE wrap_tensor_env (training/hip_tensor_env_wrappers.py), as the reference's Env sits inside
wrapping_env: the time limit counts outer steps, reward shift and scale act on the summed reward, obs_shift / obs_scale on the
float32 stack (uint8 stacks are refused there). WrappedTensorEnv.bind_engine hands the engine on to this wrapper.

The kwarg route: `hip_frame_pipe=True` on HipTensorEnvSampler / HipTensorEnvEvaluator (`frame_pipe_kwargs` below).
"""
import numbers

import numpy as np
import torch

from training.hip_acting_common import require_env_state

__all__ = ["frame_pipe_tensor_env", "FramePipeTensorEnv", "frame_pipe_kwargs"]

STATE_FORMAT = "dsact-tensor-frame-pipe-state/1"
MAX_FRAME_STACK = 64
GRAY_WEIGHTS = (0.299, 0.587, 0.114)


def _count(value, name, most=None):
    """frame_stack / action_repeat as an int >= 1 (None: 1)"""
    if value is None:
        return 1
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (numbers.Integral, np.integer)) or int(value) < 1:
        raise ValueError("%s must be an integer >= 1 (got %r)" % (name, value))
    if most is not None and int(value) > most:
        raise ValueError("%s must be <= %d (got %r)" % (name, most, value))
    return int(value)


def frame_pipe_tensor_env(env, gray=None, frame_stack=None, action_repeat=None):
    """the reference's gray / frame stack / action repeat for a batched tensor environment (the module docstring has the rules);
    `env` itself when every argument is None"""
    if gray is None and frame_stack is None and action_repeat is None:
        return env
    if gray is not None and not (isinstance(gray, str) and gray in ("chw", "hwc")):
        raise ValueError("gray must be None, 'chw' or 'hwc' (got %r)" % (gray,))
    return FramePipeTensorEnv(env, gray, _count(frame_stack, "frame_stack", MAX_FRAME_STACK), _count(action_repeat, "action_repeat"))


def _stacked_shape(row, gray, K):
    """the stacked row's shape for an inner row of shape `row`"""
    if gray is not None:
        if len(row) != 3 or row[0 if gray == "chw" else 2] != 3:
            raise ValueError("gray=%r needs 3-channel rows %s (the environment's rows are %r)"
                             % (gray, "[N, 3, H, W]" if gray == "chw" else "[N, H, W, 3]", tuple(row)))
        return (K,) + (tuple(row[1:]) if gray == "chw" else tuple(row[:2]))
    if len(row) < 1:
        raise ValueError("the environment's rows have no shape")
    return (K * int(row[0]),) + tuple(row[1:])


class FramePipeTensorEnv:
    use_fused = True      # False on an instance: the torch route whatever engine is bound

    def __init__(self, env, gray, frame_stack, action_repeat):
        self.env = env
        self._gray, self.frame_stack, self.action_repeat = gray, int(frame_stack), int(action_repeat)
        self._engine = None
        self._made = False        # the buffers below exist (made at the first reset(): a row's shape, dtype and device)
        self.stack = None         # [N, *obs_shape]: the last K rows of every environment, oldest first (the wrapper's state)
        self.ended_at = None      # int32 [N]: the inner index at which a row ended in the last outer step, -1: it did not

    def __getattr__(self, name):
        if name == "env":         # (not yet set: copy / pickle probing an empty instance)
            raise AttributeError(name)
        if name in ("obs_shape", "obs_dim"):   # (the properties below gave up: never the inner environment's UNSTACKED shape)
            raise AttributeError("%s is known after the first reset(): the inner environment names no row shape" % name)
        return getattr(self.env, name)

    @property
    def obs_shape(self):
        if self._made:
            return self._obs_shape
        inner = getattr(self.env, "obs_shape", None)
        if inner is None:
            dim = getattr(self.env, "obs_dim", None)
            if dim is None:
                raise AttributeError("obs_shape is known after the first reset(): the inner environment names no row shape")
            inner = (int(dim),)
        return _stacked_shape(tuple(int(s) for s in inner), self._gray, self.frame_stack)

    @property
    def obs_dim(self):
        return int(np.prod(self.obs_shape))

    # ---- routes --------------------------------------------------------------------------------------------------------------
    def bind_engine(self, engine):
        """the DsactEngine whose stream the environment's ops run on: from here on every inner step and every reset is followed
        by one launch (None: the torch route again). An inner environment that has `bind_engine` is handed the engine too."""
        self._engine = engine
        if callable(getattr(self.env, "bind_engine", None)):
            self.env.bind_engine(engine)

    @property
    def fused(self):
        return self._engine is not None and bool(self.use_fused)

    def _make(self, rows):
        """once: the wrapper's own tensors, for inner rows like `rows`[N, ...]"""
        n, dev = int(self.env.num_envs), rows.device
        if int(rows.shape[0]) != n:
            raise ValueError("the environment returned %d rows, num_envs is %d" % (int(rows.shape[0]), n))
        shape = _stacked_shape(tuple(int(s) for s in rows.shape[1:]), self._gray, self.frame_stack)
        if self._gray is not None and rows.dtype not in (torch.uint8, torch.float32):
            raise TypeError("gray needs uint8 (0..255) or float32 pixel values (the environment returned %s)" % rows.dtype)
        self._in_dtype = rows.dtype
        dt = torch.float32 if self._gray is not None else rows.dtype
        self.stack, self._obs2_out, self._obs_out = (torch.zeros((n,) + shape, dtype=dt, device=dev) for _ in range(3))
        self._rew_out, self._acc = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev)
        self._term_out, self._trunc_out, self._alive, self._done = (torch.zeros(n, dtype=torch.bool, device=dev) for _ in range(4))
        self.ended_at = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self._flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._slots = self.stack.view(n, self.frame_stack, -1)        # [N, K, P]: what both routes index
        self._n, self._obs_shape, self._made = n, shape, True

    def _on_engine_stream(self, t):
        """the fused launches go to the engine's stream: the inner environment's ops must have been issued there too (under
        `torch.cuda.stream(engine.torch_stream)`, as sampler and evaluator do), or the launch would read rows not yet written"""
        if t.is_cuda and torch.cuda.current_stream(t.device).cuda_stream != self._engine.stream_ptr:
            raise RuntimeError("a FramePipeTensorEnv bound to an engine must be stepped and reset under torch.cuda.stream(engine.torch_stream)")

    def _device_input(self, t, dtypes, name):
        """a tensor of the inner environment as the fused route takes it: on the stack's device, contiguous (made so where it is
        not), of one of `dtypes`; anything else is an error -- the route never changes quietly"""
        if t.dtype not in dtypes or t.device != self.stack.device:
            raise TypeError("the fused frame-pipe route needs %s as %s on %s (the environment returned %s on %s)"
                            % (name, " or ".join(str(d) for d in dtypes), self.stack.device, t.dtype, t.device))
        return t if t.is_contiguous() else t.contiguous()

    def _check_rows(self, raw):
        if raw.dtype != self._in_dtype or int(raw.shape[0]) != self._n or int(raw[0].numel()) != self._in_elems():
            raise ValueError("the environment's rows changed: %s %r, the first reset() returned %s rows of %d elements"
                             % (raw.dtype, tuple(raw.shape), self._in_dtype, self._in_elems()))

    def _in_elems(self):
        return int(self._slots.shape[2]) * (3 if self._gray is not None else 1)

    def _new_rows(self, raw):
        """the torch route's newest slot [N, P] of inner rows `raw`"""
        if self._gray is None:
            return raw.reshape(self._n, -1)
        r, g, b = (raw[:, 0], raw[:, 1], raw[:, 2]) if self._gray == "chw" else (raw[..., 0], raw[..., 1], raw[..., 2])
        x = r.to(torch.float64).mul_(GRAY_WEIGHTS[0])                 # (to(float64) of uint8 / float32 rows is a new tensor)
        x.add_(g.to(torch.float64).mul_(GRAY_WEIGHTS[1]))
        x.add_(b.to(torch.float64).mul_(GRAY_WEIGHTS[2]))
        x.div_(128.0).sub_(1.0)
        return x.to(torch.float32).reshape(self._n, -1)

    # ---- the protocol --------------------------------------------------------------------------------------------------------
    def reset(self, mask=None):
        raw = self.env.reset() if mask is None else self.env.reset(mask)
        if not self._made:
            self._make(raw)
        self._check_rows(raw)
        if self.fused:
            self._on_engine_stream(raw)
            m = None if mask is None else self._device_input(mask, (torch.bool, torch.uint8), "the reset mask")
            self._engine.frame_pipe_reset(self._n, self.frame_stack, self._gray, self._device_input(raw, self._raw_dtypes(), "frames"),
                                          m, self.stack, self._obs_out)
        else:
            new = self._new_rows(raw)[:, None, :]
            if mask is None:
                self._slots.copy_(new.expand_as(self._slots))
            else:
                self._slots.copy_(torch.where(mask.to(torch.bool)[:, None, None], new, self._slots))
            self._obs_out.copy_(self.stack)
        return self._obs_out

    def _raw_dtypes(self):
        return (torch.uint8, torch.float32) if self._gray is not None else (self._in_dtype,)

    def step(self, action):
        if not self._made:
            raise RuntimeError("FramePipeTensorEnv.step before the first reset(): there is no stack to push onto")
        R, K = self.action_repeat, self.frame_stack
        fused = self.fused
        if fused and self._in_dtype not in (torch.uint8, torch.float32):
            raise TypeError("the fused frame-pipe route needs uint8 or float32 rows (the environment's are %s)" % self._in_dtype)
        for j in range(R):
            raw, rew, term, trunc = self.env.step(action)
            self._check_rows(raw)
            if fused:
                self._on_engine_stream(rew)
                flag = (torch.bool, torch.uint8)
                self._engine.frame_pipe_step(
                    self._n, j, R, K, self._gray, self._device_input(raw, self._raw_dtypes(), "frames"),
                    self._device_input(rew, (torch.float32,), "rewards"), self._device_input(term, flag, "terminated"),
                    self._device_input(trunc, flag, "truncated"), self.stack, self._acc, self.ended_at, self._flags, self._obs2_out,
                    self._rew_out, self._term_out, self._trunc_out)
                continue
            new, top = self._new_rows(raw), self._slots[:, K - 1]
            term, trunc, rew = term.to(torch.bool), trunc.to(torch.bool), rew.to(torch.float32)
            torch.logical_or(term, trunc, out=self._done)
            if j == 0:                    # every row is alive: shift, push, start the sum
                if K > 1:
                    self._slots[:, :K - 1].copy_(self._slots[:, 1:].clone())
                top.copy_(new)
                self._acc.copy_(rew)
                self._term_out.copy_(term)
                self._trunc_out.copy_(trunc)
                self.ended_at.fill_(-1).masked_fill_(self._done, 0)
                torch.logical_not(self._done, out=self._alive)
            else:                         # rows alive at the start of j: overwrite the newest slot, add, keep the ending flags
                top.copy_(torch.where(self._alive[:, None], new, top))
                self._acc.copy_(torch.where(self._alive, self._acc + rew, self._acc))
                self._term_out.copy_(torch.where(self._alive, term, self._term_out))
                self._trunc_out.copy_(torch.where(self._alive, trunc, self._trunc_out))
                self._done.logical_and_(self._alive)
                self.ended_at.masked_fill_(self._done, j)
                self._alive.logical_and_(self._done.logical_not_())
        if not fused:
            self._rew_out.copy_(self._acc)
            self._obs2_out.copy_(self.stack)
        return self._obs2_out, self._rew_out, self._term_out, self._trunc_out

    # ---- run state -----------------------------------------------------------------------------------------------------------
    def _params(self):
        """the wrapper's parameters as plain Python values (what load_state_dict compares)"""
        return {"gray": self._gray, "frame_stack": self.frame_stack, "action_repeat": self.action_repeat}

    def state_dict(self):
        inner = require_env_state(self.env, "FramePipeTensorEnv.state_dict")
        if not self._made:
            raise RuntimeError("FramePipeTensorEnv.state_dict before the first reset(): there is no stack to save")
        return {"format": STATE_FORMAT, "params": self._params(), "stack": self.stack.detach().cpu().clone(), "inner": inner.state_dict()}

    def load_state_dict(self, sd):
        inner = require_env_state(self.env, "FramePipeTensorEnv.load_state_dict")
        if not isinstance(sd, dict) or sd.get("format") != STATE_FORMAT:
            raise ValueError("not a %s object" % STATE_FORMAT)
        if sd.get("params") != self._params():
            raise ValueError("the saved environment's pipeline was %r, this one's is %r: the resumed run would differ"
                             % (sd.get("params"), self._params()))
        if not self._made:
            raise RuntimeError("FramePipeTensorEnv.load_state_dict before the first reset(): call reset() first")
        saved = sd["stack"]
        if tuple(saved.shape) != tuple(self.stack.shape) or saved.dtype != self.stack.dtype:
            raise ValueError("the saved stack is %s %r, this wrapper's %s %r"
                             % (saved.dtype, tuple(saved.shape), self.stack.dtype, tuple(self.stack.shape)))
        self.stack.copy_(saved.to(self.stack.device))
        inner.load_state_dict(sd["inner"])


def frame_pipe_kwargs(kwargs, who):
    """`hip_frame_pipe` of HipTensorEnvSampler / HipTensorEnvEvaluator: None when the kwarg is off (the default), else the
    arguments of frame_pipe_tensor_env taken from the flat argument dict -- `frame_gray`, `frame_stack`, `action_repeat`. The
    evaluator keeps the repeat: the reference's Evaluator drops only the generic repeat_num wrapper, CarRacing's built-in repeat
    stays. Refused (ValueError): a non-bool value; True with none of the three set."""
    on = kwargs.get("hip_frame_pipe", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError("hip_frame_pipe must be True or False, got %r" % (on,))
    if not on:
        return None
    args = {"gray": kwargs.get("frame_gray"), "frame_stack": kwargs.get("frame_stack"), "action_repeat": kwargs.get("action_repeat")}
    if all(v is None for v in args.values()):
        raise ValueError("%s: hip_frame_pipe=True with none of frame_gray, frame_stack, action_repeat set does nothing, drop it" % who)
    return args
