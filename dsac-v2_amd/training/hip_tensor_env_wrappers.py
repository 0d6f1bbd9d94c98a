"""wrap_tensor_env -- the reference's environment wrappers (utils/wrapping_env.py:77-120) for BATCHED TENSOR ENVIRONMENTS, one
launch behind `step` and one behind `reset`.

The reference puts every environment it builds through `wrapping_env(env, max_episode_steps, reward_shift, reward_scale,
obs_shift, obs_scale)`: gym's TimeLimit, ShapingRewardData `(r + shift) * scale` and ScaleObservationData `(obs + shift) * scale`.
`wrap_tensor_env` takes the same arguments for an environment that speaks the tensor-environment protocol of
training/hip_tensor_sampler.py and returns a WrappedTensorEnv that speaks it too, so sampler, evaluator, captured graphs,
eval_save, episode statistics and run states work with it unchanged. With every argument None it returns `env` itself.

The rules are the reference's (wrapping_env.py:101-118). Values are float32; every parameter is cast with np.float32 once, on
the host.
  reward       reward = (r + shift) * scale, two separately rounded fp32 operations. A missing one of the pair defaults to 0.0 /
               1.0. With neither given the inner reward tensor is returned as it is.
  observation  obs = (raw + shift) * scale, on step's obs2, on reset() and on EVERY row reset(mask) returns (the inner
               environment returns raw rows for restarted and untouched rows alike). shift / scale are scalars, lists or arrays of
               one row's shape ([O], or [C, H, W] for float32 frames), kept as two device arrays of one row's length. uint8 frames
               hold codes, not values: obs_shift / obs_scale on an environment whose first reset() returns uint8 is a
               NotImplementedError; without them such frames pass through untouched (the same tensor, no copy).
  time limit   one int32 [N] tensor `elapsed`, owned by the wrapper and only ever updated in place. step: elapsed =
               min(elapsed + 1, M) (saturating: a row that is never reset cannot overflow), hit = elapsed >= M, `terminated` is
               the inner tensor as it is, truncated_out = truncated_in | (hit & ~terminated) -- gym 0.23's
               info["TimeLimit.truncated"] = not done. An inner environment's own truncation is KEPT (the OR); nested TimeLimits
               in gym would drop the inner flag in the one step where both fire, because the outer wrapper overwrites the info
               key. reset() zeroes elapsed, reset(mask) zeroes it where the mask is set. M is an integer >= 1.
               UNLIKE THE REFERENCE (wrapping_env.py:102-103) an environment's own `max_episode_steps` attribute is NOT picked up
               as the default: a tensor environment that carries the attribute enforces that limit itself.

Outputs are wrapper-owned tensors, allocated once (at the first reset(), when a row's shape, dtype and device are known).
step's obs2 and reset's obs live in different buffers, so a caller that still reads one while the other is written -- the tensor
evaluator's in-place reads under hip_graph_eval -- stays valid.

Forwarded: `capture_safe` is the inner environment's value (the wrapper itself keeps the promise: in-place state, no allocation
that outlives a call, nothing on the host, torch's current stream); `num_envs`, `action_low`, `action_high` and every other
attribute forward to the inner environment; `max_episode_steps` is M when a limit is set, so the tensor evaluator's eval_save
finds its default step bound.

Two routes, bit for bit equal:
  torch route  in-place / out= torch ops only, about a dozen small launches per lockstep step. CPU and GPU; the restatement the
               tests compare against.
  fused route  dsact_env_wrap_step / dsact_env_wrap_reset (k_env_wrap_step / k_env_wrap_reset, csrc/dsact_kernels.h): ONE launch
               each. Selected by `bind_engine(engine)` with a DsactEngine on the tensors' GPU; `fused` tells which route is
               active. HipTensorEnvSampler._setup and the tensor evaluator's per-engine set-up call bind_engine where an
               environment has the method. The launches go to the engine's stream, so a bound wrapper is stepped and reset
               under `torch.cuda.stream(engine.torch_stream)` (as both classes do; anything else is a RuntimeError). On the fused route a tensor the inner environment returns in another dtype or on
               another device is an error, never a quiet change of route. `use_fused = False` on an instance keeps the torch
               route whatever is bound (measurements, and the tests' restatement inside a sampler).

Run state: state_dict() -> {"format", "params", "elapsed" (CPU), "inner": env.state_dict()}; an inner environment without the
method raises require_env_state's NotImplementedError. load_state_dict refuses other parameters (ValueError) and copies
`elapsed` into place, so the sampler's run_state() / load_run_state() resume a wrapped run bit for bit.

Refused by wrap_tensor_env before any environment call (ValueError): a non-integer or < 1 max_episode_steps, a non-finite shift
or scale, a shift / scale array of another shape than a row -- checked against the other array of the pair and against the
environment's `obs_shape` / `obs_dim` attribute where it has one, and once more against the first reset()'s rows.

The kwarg route: `hip_env_wrap=True` on HipTensorEnvSampler / HipTensorEnvEvaluator (`env_wrap_kwargs` below).
"""
import numbers

import numpy as np
import torch

from training.hip_acting_common import require_env_state

__all__ = ["wrap_tensor_env", "WrappedTensorEnv", "env_wrap_kwargs"]

STATE_FORMAT = "dsact-tensor-env-wrap-state/1"


def _f32_param(value, name):
    """a shift / scale as a float32 array (shape () for a scalar), finite"""
    try:
        arr = np.asarray(value, dtype=np.float32)
    except (TypeError, ValueError) as ex:
        raise ValueError("%s must be a number, a list or an array (got %r)" % (name, value)) from ex
    if not np.isfinite(arr).all():
        raise ValueError("%s must be finite (got %r)" % (name, value))
    return arr


def _row_shape_of(env):
    """the shape of one observation row where the environment names it (obs_shape, else obs_dim), else None"""
    shape = getattr(env, "obs_shape", None)
    if shape is not None:
        return tuple(int(s) for s in shape)
    dim = getattr(env, "obs_dim", None)
    return None if dim is None else (int(dim),)


def wrap_tensor_env(env, max_episode_steps=None, reward_shift=None, reward_scale=None, obs_shift=None, obs_scale=None):
    """the reference's wrapping_env for a batched tensor environment (the module docstring has the rules); `env` itself when every
    argument is None"""
    if max_episode_steps is None and reward_shift is None and reward_scale is None and obs_shift is None and obs_scale is None:
        return env
    limit = None
    if max_episode_steps is not None:
        if isinstance(max_episode_steps, (bool, np.bool_)) or not isinstance(max_episode_steps, (numbers.Integral, np.integer)):
            raise ValueError("max_episode_steps must be an integer >= 1 (got %r)" % (max_episode_steps,))
        limit = int(max_episode_steps)
        if not 1 <= limit <= (1 << 31) - 2:       # (elapsed + 1 <= M + 1 must fit int32)
            raise ValueError("max_episode_steps must be an integer in [1, 2^31 - 2] (got %r)" % (max_episode_steps,))
    reward = None
    if reward_shift is not None or reward_scale is not None:
        pair = []
        for value, default, name in ((reward_shift, 0.0, "reward_shift"), (reward_scale, 1.0, "reward_scale")):
            arr = _f32_param(default if value is None else value, name)
            if arr.size != 1:
                raise ValueError("%s must be one number (got %r)" % (name, value))
            pair.append(np.float32(arr.reshape(-1)[0]))
        reward = tuple(pair)
    obs = None
    if obs_shift is not None or obs_scale is not None:
        shift = _f32_param(0.0 if obs_shift is None else obs_shift, "obs_shift")
        scale = _f32_param(1.0 if obs_scale is None else obs_scale, "obs_scale")
        named = _row_shape_of(env)
        shapes = [a.shape for a in (shift, scale) if a.shape != ()]
        for s in shapes:
            if s != shapes[0] or (named is not None and s != named):
                raise ValueError("obs_shift / obs_scale must be scalars or arrays of one observation row's shape%s (got %r and %r)"
                                 % ("" if named is None else " %r" % (named,), shift.shape, scale.shape))
        obs = (shift, scale)
    return WrappedTensorEnv(env, limit, reward, obs)


class WrappedTensorEnv:
    use_fused = True      # False on an instance: the torch route whatever engine is bound

    def __init__(self, env, limit, reward, obs):
        self.env = env
        self._limit, self._reward, self._obs_params = limit, reward, obs
        if limit is not None:
            self.max_episode_steps = limit
        self._engine = None
        self._made = False        # the buffers below exist (made at the first reset(): a row's shape, dtype and device)
        self._scale_obs = False   # the observation part is on (decided with the first rows: uint8 frames are refused)
        self.elapsed = None       # int32 [N], steps into the running episode (saturating at the limit)

    def __getattr__(self, name):
        if name == "env":         # (not yet set: copy / pickle probing an empty instance)
            raise AttributeError(name)
        return getattr(self.env, name)

    # ---- routes --------------------------------------------------------------------------------------------------------------
    def bind_engine(self, engine):
        """the DsactEngine whose stream the environment's ops run on: from here on step and reset are one launch each (None: the
        torch route again). An inner environment that has `bind_engine` (training/hip_tensor_frame_pipe.py: the pipeline sits inside
        this wrapper) is handed the engine too."""
        self._engine = engine
        if callable(getattr(self.env, "bind_engine", None)):
            self.env.bind_engine(engine)

    @property
    def fused(self):
        return self._engine is not None and bool(self.use_fused)

    def _make(self, rows):
        """once: the wrapper's own tensors, for rows like `rows`[N, ...]"""
        n, dev = int(self.env.num_envs), rows.device
        if int(rows.shape[0]) != n:
            raise ValueError("the environment returned %d rows, num_envs is %d" % (int(rows.shape[0]), n))
        row = tuple(rows.shape[1:])
        if self._obs_params is not None:
            if rows.dtype == torch.uint8:
                raise NotImplementedError("obs_shift / obs_scale on uint8 frames: the bytes are codes into a codebook, not values; "
                                          "scale the codebook (hip_obs_codebook) instead")
            if rows.dtype != torch.float32:
                raise TypeError("obs_shift / obs_scale need float32 observations (got %s)" % rows.dtype)
            flat = []
            for arr, name in zip(self._obs_params, ("obs_shift", "obs_scale")):
                if arr.shape not in ((), row):
                    raise ValueError("%s has shape %r, an observation row %r" % (name, arr.shape, row))
                flat.append(torch.from_numpy(np.ascontiguousarray(np.broadcast_to(arr, row)).reshape(-1).copy()).to(dev))
            self._shift, self._scale = flat                          # [row's length] each: what the kernels read
            self._shift_row, self._scale_row = self._shift.view(row), self._scale.view(row)
            self._obs2_out = torch.zeros((n,) + row, dtype=torch.float32, device=dev)
            self._obs_out = torch.zeros((n,) + row, dtype=torch.float32, device=dev)
            self._scale_obs = True
        if self._reward is not None:
            self._rew_out = torch.zeros(n, dtype=torch.float32, device=dev)
        if self._limit is not None:
            self.elapsed = torch.zeros(n, dtype=torch.int32, device=dev)
            self._trunc_out, self._hit, self._alive = (torch.zeros(n, dtype=torch.bool, device=dev) for _ in range(3))
        self._n, self._made = n, True

    def _on_engine_stream(self, t):
        """the fused launches go to the engine's stream: the inner environment's ops must have been issued there too (under
        `torch.cuda.stream(engine.torch_stream)`, as sampler and evaluator do), or the launch would read rows not yet written"""
        if t.is_cuda and torch.cuda.current_stream(t.device).cuda_stream != self._engine.stream_ptr:
            raise RuntimeError("a WrappedTensorEnv bound to an engine must be stepped and reset under torch.cuda.stream(engine.torch_stream)")

    def _device_input(self, t, dtypes, name):
        """a tensor of the inner environment as the fused route takes it: contiguous (made so where it is not), of one of
        `dtypes`; anything else is an error -- the route never changes quietly"""
        if t.dtype not in dtypes:
            raise TypeError("the fused wrapper route needs %s as %s (the environment returned %s)"
                            % (name, " or ".join(str(d) for d in dtypes), t.dtype))
        return t if t.is_contiguous() else t.contiguous()

    # ---- the protocol --------------------------------------------------------------------------------------------------------
    def reset(self, mask=None):
        raw = self.env.reset() if mask is None else self.env.reset(mask)
        if not self._made:
            self._make(raw)
        limit_on = self._limit is not None
        if not self._scale_obs and not limit_on:
            return raw
        if self.fused:
            self._on_engine_stream(raw)
            m = None
            if limit_on and mask is not None:
                m = self._device_input(mask, (torch.bool, torch.uint8), "the reset mask")
            src = self._device_input(raw, (torch.float32,), "observations") if self._scale_obs else None
            self._engine.env_wrap_reset(self._n, obs=src, mask=m, obs_shift=self._shift if self._scale_obs else None,
                                        obs_scale=self._scale if self._scale_obs else None,
                                        elapsed=self.elapsed if limit_on else None,
                                        obs_out=self._obs_out.view(src.shape) if self._scale_obs else None)
        else:
            if self._scale_obs:
                out = self._obs_out.view(raw.shape)
                torch.add(raw, self._shift_row.view(raw.shape[1:]), out=out)
                out.mul_(self._scale_row.view(raw.shape[1:]))
            if limit_on:
                if mask is None:
                    self.elapsed.zero_()
                else:
                    self.elapsed.masked_fill_(mask.to(torch.bool), 0)
        return self._obs_out.view(raw.shape) if self._scale_obs else raw

    def step(self, action):
        obs2, rew, term, trunc = self.env.step(action)
        if not self._made:
            self._make(obs2)
        limit_on, rew_on = self._limit is not None, self._reward is not None
        if self.fused:
            self._on_engine_stream(rew)
            f32, flag = (torch.float32,), (torch.bool,)
            src = self._device_input(obs2, f32, "observations") if self._scale_obs else None
            self._engine.env_wrap_step(
                self._n, obs2=src, rew=self._device_input(rew, f32, "rewards") if rew_on else None,
                terminated=self._device_input(term, flag, "terminated") if limit_on else None,
                truncated=self._device_input(trunc, flag, "truncated") if limit_on else None,
                obs_shift=self._shift if self._scale_obs else None, obs_scale=self._scale if self._scale_obs else None,
                reward_shift=self._reward[0] if rew_on else 0.0, reward_scale=self._reward[1] if rew_on else 1.0, reward_on=rew_on,
                max_episode_steps=self._limit or 0, elapsed=self.elapsed if limit_on else None,
                obs2_out=self._obs2_out.view(src.shape) if self._scale_obs else None,
                rew_out=self._rew_out if rew_on else None, truncated_out=self._trunc_out if limit_on else None)
        else:
            if self._scale_obs:
                out = self._obs2_out.view(obs2.shape)
                torch.add(obs2, self._shift_row.view(obs2.shape[1:]), out=out)
                out.mul_(self._scale_row.view(obs2.shape[1:]))
            if rew_on:
                torch.add(rew, float(self._reward[0]), out=self._rew_out)
                self._rew_out.mul_(float(self._reward[1]))
            if limit_on:
                self.elapsed.add_(1).clamp_(max=self._limit)
                torch.ge(self.elapsed, self._limit, out=self._hit)
                torch.logical_not(term, out=self._alive)
                self._hit.logical_and_(self._alive)
                torch.logical_or(trunc, self._hit, out=self._trunc_out)
        return (self._obs2_out.view(obs2.shape) if self._scale_obs else obs2, self._rew_out if rew_on else rew, term,
                self._trunc_out if limit_on else trunc)

    # ---- run state -----------------------------------------------------------------------------------------------------------
    def _params(self):
        """the wrapper's parameters as plain Python values (what load_state_dict compares)"""
        obs = None if self._obs_params is None else [[list(a.shape), a.reshape(-1).tolist()] for a in self._obs_params]
        return {"max_episode_steps": self._limit, "reward": None if self._reward is None else [float(v) for v in self._reward],
                "obs": obs}

    def state_dict(self):
        inner = require_env_state(self.env, "WrappedTensorEnv.state_dict")
        if self._limit is not None and self.elapsed is None:
            raise RuntimeError("WrappedTensorEnv.state_dict before the first reset(): there is no episode to save")
        return {"format": STATE_FORMAT, "params": self._params(),
                "elapsed": None if self.elapsed is None else self.elapsed.detach().cpu().clone(), "inner": inner.state_dict()}

    def load_state_dict(self, sd):
        inner = require_env_state(self.env, "WrappedTensorEnv.load_state_dict")
        if not isinstance(sd, dict) or sd.get("format") != STATE_FORMAT:
            raise ValueError("not a %s object" % STATE_FORMAT)
        if sd.get("params") != self._params():
            raise ValueError("the saved environment was wrapped with %r, this one with %r: the resumed run would differ"
                             % (sd.get("params"), self._params()))
        if self._limit is not None:
            if self.elapsed is None:
                raise RuntimeError("WrappedTensorEnv.load_state_dict before the first reset(): call reset() first")
            saved = sd["elapsed"]
            if tuple(saved.shape) != tuple(self.elapsed.shape):
                raise ValueError("the saved elapsed counters have shape %r, this wrapper steps %r" % (tuple(saved.shape), tuple(self.elapsed.shape)))
            if int(saved.min()) < 0 or int(saved.max()) > self._limit:
                raise ValueError("the saved elapsed counters leave [0, %d]: not a state this wrapper wrote" % self._limit)
            self.elapsed.copy_(saved.to(self.elapsed.device))
        inner.load_state_dict(sd["inner"])


def env_wrap_kwargs(kwargs, who):
    """`hip_env_wrap` of HipTensorEnvSampler / HipTensorEnvEvaluator: None when the kwarg is off (the default), else the arguments
    of wrap_tensor_env taken from the flat argument dict -- max_episode_steps, reward_shift, obs_shift, obs_scale. reward_scale is
    deliberately NOT among them: the sampler multiplies by it once at the ring write (the reference applies it twice, in
    create_env and again in OffSampler.sample; who wants that product calls wrap_tensor_env(reward_scale=...) directly), and the
    reference's Evaluator clears it. Refused (ValueError): a non-bool value; True with none of the four set."""
    on = kwargs.get("hip_env_wrap", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError("hip_env_wrap must be True or False, got %r" % (on,))
    if not on:
        return None
    names = ("max_episode_steps", "reward_shift", "obs_shift", "obs_scale")
    args = {k: kwargs.get(k) for k in names}
    if all(v is None for v in args.values()):
        raise ValueError("%s: hip_env_wrap=True with none of %s set does nothing, drop it" % (who, ", ".join(args)))
    return args
