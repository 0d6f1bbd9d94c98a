"""HipTensorEnvSampler -- the sampler for BATCHED TENSOR ENVIRONMENTS: simulators that take an [N, A] action tensor on the GPU and
return [N, O] observations, rewards and done flags on the GPU (`plugin.create_sampler(sampler_name="hip_tensor_env_sampler",
env=..., ...)`).

HipVecOffSampler (training/hip_vec_sampler.py) steps N Python environments and moves every observation, action and transition
across the bus; for an environment that already lives on the device that is pure overhead. Here nothing leaves the GPU and
nothing waits: a lockstep step is ONE dsact_act_sample_device call (policy(obs) on the live weights + the distribution's sample
with noise drawn in the kernel + the clip to the action limits, csrc/dsact_act_batch.h), the environment's own step / reset,
and a few row copies -- all enqueued on the engine's stream. The returned DeviceSampleBatch goes to the replay ring with one
launch (HipReplayBuffer.add_batch -> dsact_buffer_add_device). A whole sample() costs launches only.

Environment protocol (all values float32 / bool torch tensors on the engine's device):
    env.num_envs                          N
    env.action_low / env.action_high      [A] or [N, A]
    env.reset() -> obs[N, O]              start every environment
    env.step(clipped[N, A]) -> (obs2[N, O], reward[N], terminated[N], truncated[N])
                                          obs2 is the TRUE next observation, before any reset
    env.reset(mask[N]) -> obs[N, O]       rows where the bool mask is set are restarted, the others returned as they are
The environment's torch ops are issued under `torch.cuda.stream(engine.torch_stream)`, so they are ordered with the acting
launches without any synchronisation. An environment that launches kernels of its own must launch them on torch's current
stream.

Per environment the semantics are the reference OffSampler's (training/off_sampler.py:46-84): the action is clipped to the
environment's limits, the reward is multiplied by reward_scale, a truncated step is stored as non-terminal, an environment
that ends (terminated or truncated) restarts alone. Transitions are STEP-MAJOR like HipVecOffSampler's: sample() runs S / N
lockstep steps (S = batch_size_per_sampler or sample_batch_size, a multiple of N) and transition t * N + i is environment i's
step t.

Noise: the N(0,1) draws behind Normal.sample() are made in the acting kernel -- Philox4x32-10, stream id 5, keyed by
`hip_act_seed` (default act_seed_from(seed), training/hip_replay_buffer.py) and counted by `act_step`, which starts at 0,
advances by one per lockstep step and is assignable like the buffer's `index_iteration`. Environment i's noise at step t is a
pure function of (seed, t, i, action dimension): a run is reproducible from its seeds, and independent of N. It is NOT
torch.randn's stream, so `strict_rng=True` is refused.

Exploration noise (`noise_params={"mean": ..., "std": ...}`; the reference's GaussNoise, off_sampler.py:58-65 and
explore_noise.py:17-23): `action + N(mean, std)` before the clip, drawn in the same acting kernel on a
stream of its own -- Philox stream id 6, same seed, same step counter, so nothing leaves the GPU and nothing waits. The draw of
np.random.normal(mean, std) has shape () or (1,): ONE normal per (environment, step), added to every action dimension (the
reference with scalar parameters); shape (A,): one per dimension. The ring stores the noised, un-clipped action, the environment
receives its clip, logp is the un-noised sample's. _setup hands the parameters to the engine once (set_explore_noise); without
noise_params no such call is made. It is NOT the global NumPy generator's stream (a run is reproducible from hip_act_seed instead).
Refused: a missing key or a discrete action_type (NotImplementedError); another key, another shape, a negative or non-finite
std, a non-finite mean (ValueError).

The clip: the kernel clips to the policy's action limits (dsact_set_action_limits). When the environment's limits are those
-- the usual case -- its `clipped` output is what the environment receives; otherwise the clip is made with two torch ops on
the device.

Image environments (`hip_cnn_act=True` AND an engine with the CNN acting path, DsactEngine.cnn_act): the
environment returns [N, C, H, W] frames, float32 or uint8. The [S, C, H, W] buffers take the dtype of the first env.reset(); a
uint8 frame holds codes into the coded ring's codebook (hip_obs_codebook) and the engine's calls dispatch on the dtype.

Refused (NotImplementedError / ValueError, before an environment step or an engine call is made): an unattached policy, a CNN
policy outside that gate, strict_rng=True, malformed noise_params (above), S not a multiple of N, an environment on another device than the engine. The overlapped
trainer (hip_off_async_trainer) refuses this sampler as an unknown sampler class: held-behaviour acting is not built for it.

Episode statistics (`hip_episode_stats=True`; default off: exactly the calls above): how the N TRAINING
environments' episodes are going, kept on the device. _setup starts them (dsact_track_begin: a new engine starts new
statistics), and sample() ends with ONE more launch, dsact_track_commit over the [S] reward / terminated / truncated buffers as
they are (S / N lockstep steps; the environment's own reward, before reward_scale) -- still no wait. `episode_statistics()` is
the one call that waits: it reads the per-row state (dsact_track_read) and aggregates it on the host. With
`hip_episode_stats_every=K` (K > 0) every K-th sample() makes that read itself (a clearing one) and adds `Sampler/episodes`,
`Sampler/episode return mean` / `min` / `max`, `Sampler/episode length mean` and `Sampler/terminated share` to the dict it
returns: the only case in which sample() waits. The count is `sample_calls` (0 at construction, +1 per sample(), assignable
like act_step) and includes the calls a trainer makes to warm the buffer up; a read whose dict nobody writes down is still a
clearing read. INTEGRATION.md says how to line the reads up with HipOffSerialTrainer's log iterations.

A sample() as one captured graph (`hip_graph_sample=True`; default off: exactly the calls above): the
environment carries `capture_safe = True` -- step and reset(mask) update their state tensors in place, allocate nothing that
must outlive the call, never touch the host and stay on torch's current stream. The first sample() after _setup runs eagerly
through dsact_act_sample_device_counted (the acting step is a counter in device memory + the step's offset; dsact_act_counter_add
closes the call), the second captures that body on the engine's stream and replays it, every later one is ONE replay();
dsact_track_commit stays behind the replay. A step's four row copies and the `|` are one launch (dsact_step_rows_device; for
[N, C, H, W] image rows dsact_step_frames_device, which splits a frame over several workgroups).
`act_step` stays assignable: the assignment writes the device counter too. `graph_captures` / `graph_replays` count.
Image environments under the kwarg: with hip_cnn_act=True on an image engine with the CNN acting path,
_setup opts the engine's CNN route into capture once (dsact_cnn_acting_capture: its device-resident acting calls record no event
any more, a held acting call fences itself) and the graph holds the chunks of 64 frames -- ingest, conv stack, feature scatter,
trunk, output -- of every step. Refused in the constructor: an environment without the attribute (NotImplementedError), a non-bool
value (ValueError), hip_cnn_act=True on an attached engine that is no image engine with the CNN acting path (NotImplementedError:
hip_cnn_act does nothing there, drop it) -- for a policy attached later, at the first sample(), before an environment or engine
call; at the first sample(): an engine off the GPU. A capture that raises is ended and re-raised as a RuntimeError naming the
environment.

The reference's environment wrappers (`hip_env_wrap=True`; default off: exactly the calls above): the
constructor puts the environment it resolved through training/hip_tensor_env_wrappers.wrap_tensor_env with `max_episode_steps`,
`reward_shift`, `obs_shift` and `obs_scale` from the flat argument dict -- NOT `reward_scale`, which this sampler multiplies by
once at the ring write. Refused (ValueError): a non-bool value, and True with none of the four set. _setup hands the engine to an
environment that has `bind_engine` (a wrapped one: its step and reset are then one launch each).

The reference's image pipeline (`hip_frame_pipe=True`; default off): the constructor puts the environment
through training/hip_tensor_frame_pipe.frame_pipe_tensor_env with `frame_gray` ("chw" / "hwc"), `frame_stack` and `action_repeat`
from the flat argument dict, BEFORE hip_env_wrap (the pipeline sits inside the wrappers). A batch row is then one held action: the
stacked observation, the reward summed over the repeat. Refused (ValueError): a non-bool value, and True with none of the three
set. Bound like a wrapped environment: one launch behind every inner step and one behind a reset.

sample() returns (DeviceSampleBatch, {sampler time}). The time is the HOST time of issuing the work. The batch's tensors are the
sampler's own preallocated [S, .] buffers: they are valid until the next sample() call (add_batch consumes them in stream
order before that).
"""
import math
import time

import numpy as np
import torch

from training.hip_acting_common import (check_noise_dim, engine_stream, explore_noise, hand_over, image_graph_engine, networks_of,
                                        on_stream, require_env_state, require_graph_cnn_pair, require_graph_device, require_tensor_engine,
                                        sample_batch_size, tensor_limits)
from training.hip_replay_buffer import act_seed_from
from training.hip_sampler import SAMPLER_TIME_KEY
from training.hip_tensor_env_wrappers import env_wrap_kwargs, wrap_tensor_env
from training.hip_tensor_frame_pipe import frame_pipe_kwargs, frame_pipe_tensor_env

__all__ = ["HipTensorEnvSampler", "DeviceSampleBatch", "act_noise_words", "act_noise_reference", "explore_noise_words",
           "explore_noise_reference", "aggregate_episode_rows", "EPISODE_TB_KEYS"]

ACT_STREAM = 5    # the acting noise's Philox stream id (include/dsact.h: 1 .. 3 the update noise, 4 the index draw)
EXPLORE_STREAM = 6   # the exploration noise's (dsact_set_explore_noise)
_M32 = 0xFFFFFFFF


def _philox_words(seed, step, block, stream=ACT_STREAM):
    """the four Philox4x32-10 words of counter (block, step low, step high, stream) under key = the seed's (low, high) words"""
    step &= 0xFFFFFFFFFFFFFFFF
    c0, c1, c2, c3 = block & _M32, step & _M32, step >> 32, stream
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def _philox_normals(seed, step, n_blocks, stream=ACT_STREAM):
    """float64 [n_blocks, 4]: the Box-Muller normals of counter blocks 0 .. n_blocks - 1 (uint64 lanes holding 32-bit words)"""
    step &= 0xFFFFFFFFFFFFFFFF
    m32 = np.uint64(_M32)
    c0 = np.arange(n_blocks, dtype=np.uint64) & m32
    c1, c2, c3 = (np.full_like(c0, v) for v in (step & _M32, step >> 32, stream))
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    u = [((w >> np.uint64(8)).astype(np.float64) + 0.5) / 16777216.0 for w in (c0, c1, c2, c3)]
    ra, rb = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    return np.stack([ra * np.cos(2 * np.pi * u[1]), ra * np.sin(2 * np.pi * u[1]), rb * np.cos(2 * np.pi * u[3]), rb * np.sin(2 * np.pi * u[3])], axis=1)


def explore_noise_words(seed, step, row, d, act_dim, shared):
    """act_noise_words for the exploration normal (dsact_set_explore_noise) of environment `row`, action dimension `d` at acting
    step `step`: counter (row * ceil(A/4) + (0 if shared else d // 4), step low, step high, 6), the acting seed as the key;
    element 0 if shared else d % 4 -- SHARED gives every d the normal of d = 0."""
    if shared:
        d = 0
    return _philox_words(seed, step, row * ((act_dim + 3) // 4) + d // 4, EXPLORE_STREAM), d % 4


def explore_noise_reference(seed, step, n_rows, act_dim, shared):
    """float64 [n_rows, act_dim]: act_noise_reference for the exploration normals z of rows 0 .. n_rows - 1 at `step` (the kernel
    adds fma(std, z, mean) to the sample). shared: every column of a row is that row's element 0."""
    per_row = (act_dim + 3) // 4
    z = _philox_normals(seed, step, n_rows * per_row, EXPLORE_STREAM).reshape(n_rows, per_row * 4)
    if shared:
        return np.ascontiguousarray(np.repeat(z[:, :1], act_dim, axis=1))
    return np.ascontiguousarray(z[:, :act_dim])


def act_noise_words(seed, step, row, d, act_dim):
    """(the four Philox4x32-10 words, which of the four normals) behind the in-kernel N(0,1) draw of environment `row`, action
    dimension `d` at acting step `step` -- include/dsact.h's description in Python integers (no GPU, no library call): counter
    (row * ceil(A/4) + d // 4, step low, step high, 5), key = the seed's (low, high) words; element d % 4."""
    return _philox_words(seed, step, row * ((act_dim + 3) // 4) + d // 4), d % 4


def act_noise_reference(seed, step, n_rows, act_dim):
    """float64 [n_rows, act_dim]: the normals the kernel draws for rows 0 .. n_rows - 1 at `step`, by the Box-Muller map of
    include/dsact.h evaluated in float64 on the same words (u = ((w >> 8) + 0.5) / 2^24; z0, z1 = r(u0) (cos, sin)(2 pi u1);
    z2, z3 = r(u2) (cos, sin)(2 pi u3); r(u) = sqrt(-2 ln u)). act_noise_words over whole arrays (uint64 lanes holding 32-bit
    words). The kernel evaluates the map in fp32: DESIGN.md section 15 has the measured distance."""
    per_row = (act_dim + 3) // 4
    z = _philox_normals(seed, step, n_rows * per_row)
    return np.ascontiguousarray(z.reshape(n_rows, per_row * 4)[:, :act_dim])


# hip_episode_stats_every: the keys a K-th sample() adds to its dict, and the aggregate behind each
EPISODE_TB_KEYS = (("Sampler/episodes", "episodes"), ("Sampler/episode return mean", "return_mean"),
                   ("Sampler/episode return min", "return_min"), ("Sampler/episode return max", "return_max"),
                   ("Sampler/episode length mean", "length_mean"), ("Sampler/terminated share", "terminated_share"))


def aggregate_episode_rows(rows):
    """the per-row totals of dsact_track_read ({name: array[N]}) as one dict: `episodes` (int), `terminated_share`,
    `return_mean`, `return_min`, `return_max`, `length_mean`, and `rows` (the arrays themselves, the episodes in progress
    included). The means are math.fsum of the per-row sums over the total count -- fsum is exactly rounded, so the result
    does not depend on a summation order. No finished episode: the means, min and max are nan."""
    n = int(rows["episodes"].sum())
    nan = float("nan")
    done = rows["episodes"] > 0
    return {"episodes": n,
            "terminated_share": int(rows["terminated"].sum()) / n if n else nan,
            "return_mean": math.fsum(rows["ret_sum"][done].tolist()) / n if n else nan,
            "return_min": float(rows["ret_min"][done].min()) if n else nan,
            "return_max": float(rows["ret_max"][done].max()) if n else nan,
            "length_mean": int(rows["len_sum"].sum()) / n if n else nan,
            "rows": rows}


class DeviceSampleBatch:
    """S transitions as seven device tensors -- obs[S, O], act[S, A], rew[S] (the environment's reward, NOT yet scaled),
    obs2[S, O], terminated[S], truncated[S] (bool), logp[S] -- plus `reward_scale`. HipReplayBuffer.add_batch hands
    `device_columns` to the ring in one call. Any other consumer may walk it like the reference's list of
    (obs, info, act, rew, next_obs, done, logp, next_info) tuples (training/off_sampler.py:74-84): the first such use makes ONE
    device-to-host copy of the whole batch (which waits for the stream that produced it)."""

    def __init__(self, obs, act, rew, obs2, terminated, truncated, logp, reward_scale=1, stream=None, codebook=None):
        self.obs, self.act, self.rew, self.obs2 = obs, act, rew, obs2
        self.terminated, self.truncated, self.logp = terminated, truncated, logp
        self.reward_scale = reward_scale
        self.stream = stream          # the torch stream the tensors were produced on (None: the current one)
        self.codebook = codebook      # float32 table of a byte (uint8) image batch: a walked tuple's pixel is codebook[byte]
        self._tuples = None

    @property
    def device_columns(self):
        return (self.obs, self.act, self.rew, self.obs2, self.terminated, self.truncated, self.logp)

    def __len__(self):
        return int(self.rew.shape[0])

    def _host(self):
        if self._tuples is None:
            if self.obs.dim() != 2 or self.obs.dtype != torch.float32:
                return self._host_images()
            S, O, A = len(self), self.obs.shape[1], self.act.shape[1]
            with on_stream(self.stream):
                flat = torch.cat([self.obs, self.obs2, self.act, self.rew[:, None], self.logp[:, None],
                                  self.terminated[:, None].to(torch.float32), self.truncated[:, None].to(torch.float32)], dim=1)
                h = flat.cpu().numpy()     # the one copy
            obs, obs2, act = h[:, :O], h[:, O:2 * O], h[:, 2 * O:2 * O + A]
            rew, logp, term, trunc = (h[:, 2 * O + A + k] for k in range(4))
            self._tuples = [(obs[i], {}, act[i], self.reward_scale * float(rew[i]), obs2[i], bool(term[i]) and not bool(trunc[i]),
                             logp[i], {"TimeLimit.truncated": bool(trunc[i])}) for i in range(S)]
        return self._tuples

    def _host_images(self):
        """_host for image batches ([S, C, H, W] rows and / or byte frames): the two image columns are copied as they are -- a
        byte column as bytes, decoded through the codebook on the host, so the reference's tuples come out as float32 frames"""
        S, A = len(self), self.act.shape[1]
        with on_stream(self.stream):
            narrow = torch.cat([self.act, self.rew[:, None], self.logp[:, None], self.terminated[:, None].to(torch.float32),
                                self.truncated[:, None].to(torch.float32)], dim=1)
            h, obs, obs2 = narrow.cpu().numpy(), self.obs.cpu().numpy(), self.obs2.cpu().numpy()
        if obs.dtype == np.uint8:
            if self.codebook is None:
                raise ValueError("a byte (uint8) DeviceSampleBatch needs the ring's codebook to be walked as float32 tuples")
            book = np.zeros(256, np.float32)
            book[:len(self.codebook)] = np.asarray(self.codebook, np.float32)
            obs, obs2 = book[obs], book[obs2]
        act = h[:, :A]
        rew, logp, term, trunc = (h[:, A + k] for k in range(4))
        self._tuples = [(obs[i], {}, act[i], self.reward_scale * float(rew[i]), obs2[i], bool(term[i]) and not bool(trunc[i]),
                         logp[i], {"TimeLimit.truncated": bool(trunc[i])}) for i in range(S)]
        return self._tuples

    def __iter__(self):
        return iter(self._host())

    def __getitem__(self, i):
        return self._host()[i]


class HipTensorEnvSampler:
    def __init__(self, index=0, **kwargs):
        self.noise = explore_noise(kwargs)    # None, or (mean, std, shared): drawn in the acting kernel
        if kwargs.get("strict_rng", False):
            raise ValueError("hip_tensor_env_sampler with strict_rng=True: the acting noise is drawn in the kernel (Philox), not "
                             "from torch.randn's stream; a parity run wants hip_vec_off_sampler")
        self.episode_stats = bool(kwargs.get("hip_episode_stats", False))
        every = kwargs.get("hip_episode_stats_every", 0)
        if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 0:
            raise ValueError("hip_episode_stats_every must be an integer >= 0 (sample() calls; 0: only on request), got %r" % (every,))
        if every > 0 and not self.episode_stats:
            raise ValueError("hip_episode_stats_every=%d needs hip_episode_stats=True" % every)
        self.episode_stats_every = int(every)
        self.sample_calls = 0             # sample() calls made: the K-th-call read counts these (assignable, like act_step)
        env = kwargs.get("env")
        if env is None:
            from plugin import create_env
            env = create_env(**kwargs)
        pipe = frame_pipe_kwargs(kwargs, "hip_tensor_env_sampler")   # hip_frame_pipe; None: off, the default
        if pipe is not None:
            env = frame_pipe_tensor_env(env, **pipe)                # (inside hip_env_wrap, as the reference's Env sits inside wrapping_env)
        wrap = env_wrap_kwargs(kwargs, "hip_tensor_env_sampler")   # hip_env_wrap; None: off, the default
        if wrap is not None:
            env = wrap_tensor_env(env, **wrap)
        self.env = env
        self.n_envs = int(env.num_envs)
        self.sample_batch_size = sample_batch_size(kwargs)
        if self.n_envs < 1 or self.sample_batch_size % self.n_envs:
            raise ValueError("the sample batch size %d is not a multiple of the environment's num_envs %d"
                             % (self.sample_batch_size, self.n_envs))
        self.action_type = kwargs.get("action_type", "continu")
        self.reward_scale = kwargs.get("reward_scale", 1)
        seed = kwargs.get("hip_act_seed")
        self.act_seed = int(seed) if seed is not None else act_seed_from(kwargs.get("seed"))
        if not 0 < self.act_seed < (1 << 64):
            raise ValueError("hip_act_seed must be in [1, 2^64) (0 switches the in-kernel draw off), got %r" % (seed,))
        self.cnn_act = bool(kwargs.get("hip_cnn_act", False))   # image environments on an engine with the CNN acting path
        # hip_graph_sample: sample() as one captured graph. Refused here, before any environment or engine call
        graph = kwargs.get("hip_graph_sample", False)
        if not isinstance(graph, (bool, np.bool_)):
            raise ValueError("hip_graph_sample must be True or False, got %r" % (graph,))
        self.graph_sample = bool(graph)
        if self.graph_sample and self.cnn_act and kwargs.get("networks") is not None:
            # the pair is for image engines with the CNN acting path; a policy attached later is checked
            # at the first sample(), before anything runs
            require_graph_cnn_pair("hip_graph_sample", kwargs["networks"])
        if self.graph_sample and getattr(env, "capture_safe", False) is not True:
            raise NotImplementedError("hip_graph_sample=True needs an environment with the attribute capture_safe = True (step and "
                                      "reset(mask) update their state tensors in place, allocate nothing that outlives the call, "
                                      "never touch the host and stay on torch's current stream); %s does not promise it"
                                      % type(env).__name__)
        self.graph_captures = 0           # captures made / replays issued (the capturing call makes the first replay)
        self.graph_replays = 0
        self._graph = None                # the captured sample() (torch.cuda.CUDAGraph), dropped with a new engine
        self._graph_calls = 0             # sample() calls on this engine: 0 -> eager warm-up, 1 -> capture, later -> replay
        self._graph_eng = None            # the engine whose device counter mirrors act_step
        self._one_launch_rows = True      # the row copies of a step as one launch (False: the torch copies; measurements)
        self._act_step = 0                # the acting-step counter behind the `act_step` property: one per lockstep step (assignable)
        self.total_sample_number = 0
        self._ready = None                # id of the engine the buffers / seed / clip route were set up for
        self._started = False             # env.reset() has been called
        self.networks = networks_of(kwargs)   # (the reference's throw-away container: built for its use of the torch generator)
        if kwargs.get("networks") is not None:
            check_noise_dim(self.noise, self._engine().act_dim)   # an explicit policy is checked right away

    def load_state_dict(self, state_dict):
        self.networks.load_state_dict(state_dict)

    def get_total_sample_number(self):
        return self.total_sample_number

    def _engine(self):
        """the engine behind the ATTACHED MLP policy (hip_cnn_act=True: or CNN policy with the CNN acting path); every other
        setup is refused"""
        if self.graph_sample and self.cnn_act:
            require_graph_cnn_pair("hip_graph_sample", self.networks)
        return require_tensor_engine("hip_tensor_env_sampler", self.networks, self.action_type, self.env, self.cnn_act)

    @property
    def act_step(self):
        """the acting-step counter (host mirror): one per lockstep step. With hip_graph_sample the kernels read its twin in device
        memory (dsact_act_counter_*); an assignment writes both, in stream order."""
        return self._act_step

    @act_step.setter
    def act_step(self, value):
        self._act_step = int(value)
        if self.graph_sample and self._graph_eng is not None and self._ready == id(self._graph_eng):   # (else _setup writes it)
            self._graph_eng.act_counter_set(self._act_step)

    def _setup(self, eng):
        """once per engine: the [S, .] buffers, the acting seed, the exploration noise, and whether the kernel's clip is the
        environment's"""
        N, S, O, A = self.n_envs, self.sample_batch_size, eng.obs_dim, eng.act_dim
        check_noise_dim(self.noise, A)
        dev = torch.device(eng.device)
        if self.graph_sample:
            require_graph_device("hip_graph_sample", dev)
            self._graph, self._graph_calls, self._graph_eng = None, 0, eng   # a new engine: eager, capture, replay again
        f = dict(dtype=torch.float32, device=dev)
        # the observation rows: [., O] float32; an image environment on a CNN engine keeps [., C, H, W] rows in the FRAME's dtype
        # (float32, or uint8: codes into the coded ring's codebook -- DESIGN.md section 20)
        first = None if self._started else self.env.reset()
        row, odt = (O,), torch.float32
        if getattr(eng, "conv_type", None):
            row = tuple(getattr(eng, "obs_shape", None) or first.shape[1:])
            odt = torch.uint8 if (first if first is not None else self._obs).dtype == torch.uint8 else torch.float32
        self._row = row
        self._obs_b, self._obs2_b = torch.zeros((S,) + row, dtype=odt, device=dev), torch.zeros((S,) + row, dtype=odt, device=dev)
        self._act_b, self._clip_b = torch.zeros(S, A, **f), torch.zeros(S, A, **f)
        self._rew_b, self._logp_b = torch.zeros(S, **f), torch.zeros(S, **f)
        self._term_b = torch.zeros(S, dtype=torch.bool, device=dev)
        self._trunc_b = torch.zeros(S, dtype=torch.bool, device=dev)
        if first is not None or tuple(self._obs.shape) != (N,) + row:
            self._obs = torch.zeros((N,) + row, dtype=odt, device=dev)
        self._low, self._high, self._kernel_clip = tensor_limits(self.env, eng, N)
        eng.set_act_rng(self.act_seed)
        if self.noise is not None:
            eng.set_explore_noise(self.noise[0], self.noise[1])   # (without noise_params no call is made: the handle's default is off)
        if self.episode_stats:
            eng.track_begin(N)            # (a new engine starts new statistics)
        if self.graph_sample:
            self._ended = torch.zeros(N, dtype=torch.bool, device=dev)   # terminated | truncated of a step: the mask of env.reset
            if self.cnn_act and image_graph_engine(eng):
                eng.cnn_acting_capture()                                 # the CNN route's opt-in to capture
            eng.act_counter_set(self._act_step)                          # the device twin of act_step
        if first is not None:
            self._obs.copy_(first.reshape((N,) + row))
            self._started = True
        if callable(getattr(self.env, "bind_engine", None)):
            # a wrapped environment's step / reset as one launch each on the engine's stream -- bound behind
            # the first reset(), which ran on torch's current stream
            self.env.bind_engine(eng)
        hand_over(eng)   # (the only wait this sampler ever makes, once)
        self._ready = id(eng)

    def _graph_body(self, eng):
        """hip_graph_sample: the S / N lockstep steps of one sample() on torch's current stream -- issued once eagerly, once under
        capture, and replayed from then on. sample()'s own loop, except that the acting step is the device counter + t
        (act_sample_device_counted), the four row copies and the `|` are one launch (step_rows_device; step_frames_device for
        [N, C, H, W] image rows, uint8 or float32; the torch copies where the environment hands back anything but contiguous
        tensors of those dtypes / bool) and act_counter_add(S / N) closes it."""
        N, S = self.n_envs, self.sample_batch_size
        env = self.env
        obs_b, obs2_b, act_b, clip_b = self._obs_b, self._obs2_b, self._act_b, self._clip_b
        rew_b, logp_b, term_b, trunc_b = self._rew_b, self._logp_b, self._term_b, self._trunc_b
        obs_b[0:N].copy_(self._obs)
        for t in range(S // N):
            r0, r1 = t * N, (t + 1) * N
            eng.act_sample_device_counted(obs_b[r0:r1], t, act_b[r0:r1], clip_b[r0:r1], logp_b[r0:r1])
            if not self._kernel_clip:
                torch.minimum(torch.maximum(act_b[r0:r1], self._low), self._high, out=clip_b[r0:r1])
            obs2, rew, term, trunc = env.step(clip_b[r0:r1])
            obs2 = obs2.reshape((N,) + self._row)
            one = (self._one_launch_rows and rew.dtype == torch.float32 and term.dtype == torch.bool
                   and trunc.dtype == torch.bool and tuple(rew.shape) == tuple(term.shape) == tuple(trunc.shape) == (N,)
                   and obs2.is_contiguous() and rew.is_contiguous() and term.is_contiguous() and trunc.is_contiguous())
            if one and obs2.dim() == 2 and obs2.dtype == torch.float32:
                eng.step_rows_device(obs2, rew, term, trunc, obs2_b[r0:r1], rew_b[r0:r1], term_b[r0:r1], trunc_b[r0:r1], self._ended)
                ended = self._ended
            elif one and obs2.dim() == 4 and obs2.dtype in (torch.uint8, torch.float32) and obs2.dtype == obs2_b.dtype:
                # image rows: a frame is split over several workgroups (row_bytes = the frame's byte size)
                eng.step_frames_device(obs2, rew, term, trunc, obs2_b[r0:r1], rew_b[r0:r1], term_b[r0:r1], trunc_b[r0:r1], self._ended)
                ended = self._ended
            else:
                obs2_b[r0:r1].copy_(obs2)
                rew_b[r0:r1].copy_(rew)
                term_b[r0:r1].copy_(term)
                trunc_b[r0:r1].copy_(trunc)
                ended = term_b[r0:r1] | trunc_b[r0:r1]
            nxt = env.reset(ended)
            (obs_b[r1:r1 + N] if r1 < S else self._obs).copy_(nxt.reshape((N,) + self._row))
        eng.act_counter_add(S // N)

    def _graph_sample(self, eng, stream):
        """one sample() of a hip_graph_sample sampler: the first call on an engine runs _graph_body eagerly (the warm-up: it makes
        the library's lazy allocations), the second captures it into a graph on the engine's stream -- one linear chain -- and
        replays it, every later call is one replay. A capture that raises is ended and reported; nothing is retried."""
        if self._graph_calls == 0:
            self._graph_body(eng)
        else:
            if self._graph is None:
                graph = torch.cuda.CUDAGraph()
                try:
                    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):   # (its exit ends the capture)
                        self._graph_body(eng)
                except Exception as ex:
                    raise RuntimeError("hip_graph_sample: capturing sample() failed with the environment %s (%s: %s). capture_safe = "
                                       "True promises that step and reset(mask) update state in place, never touch the host and "
                                       "stay on torch's current stream; build the sampler without hip_graph_sample for this "
                                       "environment" % (type(self.env).__name__, type(ex).__name__, ex)) from ex
                self._graph = graph
                self.graph_captures += 1
            self._graph.replay()
            self.graph_replays += 1
        self._graph_calls += 1
        self._act_step += self.sample_batch_size // self.n_envs   # (the device counter moved itself: act_counter_add)

    def sample(self):
        eng = self._engine()
        t0 = time.perf_counter()
        if self._ready != id(eng):
            self._setup(eng)
        N, S = self.n_envs, self.sample_batch_size
        env = self.env
        obs_b, obs2_b, act_b, clip_b = self._obs_b, self._obs2_b, self._act_b, self._clip_b
        rew_b, logp_b, term_b, trunc_b = self._rew_b, self._logp_b, self._term_b, self._trunc_b
        stream = engine_stream(eng)
        with on_stream(stream), torch.no_grad():
            if self.graph_sample:
                self._graph_sample(eng, stream)       # (the steps below as one eager call, then one captured graph)
            else:
                obs_b[0:N].copy_(self._obs)
            for t in range(0 if self.graph_sample else S // N):
                r0, r1 = t * N, (t + 1) * N
                eng.act_sample_device(obs_b[r0:r1], None, self.act_step, act_b[r0:r1], clip_b[r0:r1], logp_b[r0:r1])
                self.act_step += 1
                if not self._kernel_clip:
                    torch.minimum(torch.maximum(act_b[r0:r1], self._low), self._high, out=clip_b[r0:r1])
                obs2, rew, term, trunc = env.step(clip_b[r0:r1])
                obs2_b[r0:r1].copy_(obs2.reshape((N,) + self._row))
                rew_b[r0:r1].copy_(rew)
                term_b[r0:r1].copy_(term)
                trunc_b[r0:r1].copy_(trunc)
                # the next step's observations: this step's, with every environment that ended restarted on its own
                nxt = env.reset(term_b[r0:r1] | trunc_b[r0:r1])
                (obs_b[r1:r1 + N] if r1 < S else self._obs).copy_(nxt.reshape((N,) + self._row))
            if self.episode_stats:
                eng.track_commit(rew_b, term_b, trunc_b, S // N)    # the S / N steps in one launch
        self.total_sample_number += S
        self.sample_calls += 1
        batch = DeviceSampleBatch(obs_b, act_b, rew_b, obs2_b, term_b, trunc_b, logp_b, self.reward_scale, stream=stream,
                                  codebook=getattr(eng, "codebook", None))
        tb = {}
        if self.episode_stats_every and self.sample_calls % self.episode_stats_every == 0:
            stats = self.episode_statistics(clear=True)             # (the only wait sample() ever makes)
            tb = {key: stats[name] for key, name in EPISODE_TB_KEYS}
        tb[SAMPLER_TIME_KEY] = (time.perf_counter() - t0) * 1000
        return batch, tb

    RUN_STATE_FORMAT = "dsact-tensor-sampler-state/1"

    def _noise_state(self):
        """the parsed noise_params as run_state() carries them: None, or (mean list, std list, shared) in float64"""
        if self.noise is None:
            return None
        return (np.asarray(self.noise[0], np.float64).reshape(-1).tolist(), np.asarray(self.noise[1], np.float64).reshape(-1).tolist(),
                bool(self.noise[2]))

    def run_state(self):
        """What a resumed run needs of this sampler (HipOffSerialTrainer's hip_save_run_state): the counters
        act_step, sample_calls and total_sample_number, the current [N, O] observations as a CPU tensor, and the environment's
        state_dict(). Waits for the engine's stream. The acting noise needs nothing: it is a function of (hip_act_seed,
        act_step, row). Episode statistics (hip_episode_stats) are NOT carried: they start anew after load_run_state."""
        env = require_env_state(self.env, "hip_tensor_env_sampler.run_state")
        eng = self._engine()
        if self._ready != id(eng):
            self._setup(eng)
        with on_stream(engine_stream(eng)), torch.no_grad():
            obs = self._obs.detach().cpu().clone()
            env_sd = env.state_dict()
        eng.sync()
        return {"format": self.RUN_STATE_FORMAT, "act_step": int(self.act_step), "sample_calls": int(self.sample_calls),
                "total_sample_number": int(self.total_sample_number), "act_seed": int(self.act_seed), "obs": obs, "env": env_sd,
                "explore_noise": self._noise_state()}

    def load_run_state(self, sd):
        """restores what run_state() saved (named so that it cannot be mistaken for load_state_dict(networks))"""
        env = require_env_state(self.env, "hip_tensor_env_sampler.load_run_state")
        if sd.get("format") != self.RUN_STATE_FORMAT:
            raise ValueError("not a %s object" % self.RUN_STATE_FORMAT)
        if int(sd.get("act_seed", self.act_seed)) != int(self.act_seed):
            raise ValueError("the saved sampler drew its acting noise with hip_act_seed %#x, this one with %#x: the resumed run would "
                             "act differently" % (int(sd["act_seed"]), int(self.act_seed)))
        saved = sd.get("explore_noise")   # (a state saved before noise_params was served has no such key: no noise)
        saved = None if saved is None else (list(saved[0]), list(saved[1]), bool(saved[2]))
        if saved != self._noise_state():
            raise ValueError("the saved sampler explored with noise_params (mean, std, shared) = %r, this one with %r: the resumed "
                             "run would act differently" % (saved, self._noise_state()))
        eng = self._engine()
        if self._ready != id(eng):
            self._setup(eng)
        if tuple(sd["obs"].shape) != tuple(self._obs.shape):
            raise ValueError("the saved observations have shape %r, this sampler steps %r" % (tuple(sd["obs"].shape), tuple(self._obs.shape)))
        with on_stream(engine_stream(eng)), torch.no_grad():
            self._obs.copy_(sd["obs"].to(self._obs.device))
            env.load_state_dict(sd["env"])
        eng.sync()
        self.act_step, self.sample_calls = int(sd["act_step"]), int(sd["sample_calls"])
        self.total_sample_number = int(sd["total_sample_number"])

    def episode_statistics(self, clear=True):
        """the training environments' finished episodes since the last clearing read (or since the statistics began), over all
        rows: aggregate_episode_rows of ONE dsact_track_read, which waits for the engine's stream. clear: the totals start again
        (an episode in progress is never cut: it is counted whole when it ends). Before the first sample() the set-up of
        sample() is made here, and the answer is zero episodes."""
        if not self.episode_stats:
            raise RuntimeError("episode_statistics() needs a sampler built with hip_episode_stats=True")
        eng = self._engine()
        if self._ready != id(eng):
            self._setup(eng)
        return aggregate_episode_rows(eng.track_read(clear))
