"""HipTensorEnvEvaluator -- the evaluator for BATCHED TENSOR ENVIRONMENTS: the evaluation episodes of training/evaluator.py:34-84
on a simulator that keeps N environments as tensors on the GPU (`plugin.create_evaluator(evaluator_name=
"hip_tensor_env_evaluator", eval_env=..., ...)`). It is HipTensorEnvSampler's counterpart
(training/hip_tensor_sampler.py): with both, a tensor-environment run trains and evaluates without a per-row adapter.

HipEvaluator and HipVecEvaluator step Python objects, copy every observation to the device and wait for every action. Here a
lockstep step is launches only, all enqueued on the engine's stream:
    dsact_act_mode_device   policy(obs) on the live weights + the action distribution's mode() (csrc/dsact_act_batch.h)
    env.step(action)        the environment's own torch ops
    dsact_eval_commit       the episode bookkeeping of all N rows in one launch (k_eval_commit, csrc/dsact_kernels.h)
    env.reset(ended)        rows whose episode ended restart alone
and the host waits once every `hip_eval_poll_steps` lockstep steps (dsact_eval_poll: the number of episodes not finished yet).

Environment protocol: exactly the sampler's (float32 / bool torch tensors on the engine's device) --
    env.num_envs                          N
    env.action_low / env.action_high      [A] or [N, A]
    env.reset() -> obs[N, O]              start every environment
    env.step(action[N, A]) -> (obs2[N, O], reward[N], terminated[N], truncated[N])
    env.reset(mask[N]) -> obs[N, O]       rows where the bool mask is set are restarted, the others returned as they are
The environment is `eval_env`, else `env`, else `create_env(**kwargs)`. It must be a DIFFERENT INSTANCE from the sampler's:
an evaluation calls reset() and steps every row, which would throw away the episodes the sampler is in the middle of. Its
torch ops are issued under `torch.cuda.stream(engine.torch_stream)`; an environment that launches kernels of its own must
launch them on torch's current stream.

Episode order: episode e (0 .. num_eval_episode - 1) runs on environment e % N, and an environment plays its episodes in index
order -- HipVecEvaluator's rule. An episode ends on `terminated | truncated`.

Rows that have finished: a row with no episode left keeps stepping (and is restarted when it ends, so the simulator is never
stepped past a terminal state) and counts nothing. The result is therefore a pure function of the weights and the environment,
never of the poll period; up to hip_eval_poll_steps - 1 lockstep steps are wasted at the end.

Returns: an episode's return is the float64 sum of its float32 rewards in step order, accumulated on the device. It is NOT Python's
built-in `sum` (the reference's `sum(reward_list)`, evaluator.py:74): from Python 3.12 on `sum` compensates a float sum
(Neumaier), so a restatement adds the rewards one by one in float64. The result
of run_evaluation is np.mean(returns) in episode-index order (evaluator.py:77-81).

The clip: act_mode is inside the policy's action limits already. When the environment's limits are not the policy's, the
action is clipped to the environment's with two torch ops on the device, as in the sampler.

hip_eval_poll_steps (default 16): lockstep steps between two waits. hip_eval_max_steps (default 100 000): an evaluation that
has not finished after that many lockstep steps raises RuntimeError (the handle stays usable) -- an environment that never ends
an episode must not spin on the GPU forever.

Image environments (`hip_cnn_act=True` AND an engine with the CNN acting path): [N, C, H, W] frames, float32
or uint8 codes into the coded ring's codebook; the observation buffer takes the dtype of the first env.reset().

Refused (NotImplementedError / ValueError, before an environment or engine call is made): an unattached policy, a CNN policy
outside that gate,
non-continuous actions, an environment on another device than the engine, num_eval_episode < 1, hip_eval_poll_steps < 1.

The poll windows as one captured graph (`hip_graph_eval=True`; default off: exactly the calls above): the
environment carries `capture_safe = True`, as for the sampler's hip_graph_sample. A window is hip_eval_poll_steps lockstep
steps -- deterministic acting draws no noise, so it is the same launch sequence every time. Windows are counted per engine,
across run_evaluation calls: the first runs eagerly (it makes the library's lazy allocations), the second is captured on the
engine's stream as one linear chain and replayed, every later one is ONE replay(); dsact_eval_begin, the full env.reset() and
dsact_eval_poll stay outside the graph, and a remainder shorter than a window (hip_eval_max_steps) runs eagerly. On this route
eval_commit reads the environment's reward / terminated / truncated tensors where they are, and a step's acting call reads the
previous reset's result in place; the evaluator's observation buffer is written once per window. The graph holds the addresses of
the library's bookkeeping arrays: it is dropped (and the count restarts) on a new engine and when the engine's
`eval_state_gen` is no longer the one it was captured under -- another evaluator's larger dsact_eval_begin reallocated them.
`graph_captures` / `graph_replays` count. Image environments under the kwarg: with hip_cnn_act=True on an
image engine with the CNN acting path, _setup opts the engine's CNN route into capture once (dsact_cnn_acting_capture) and a
window holds the CNN acting forward of every step; the acting call reads the previous reset's frames in place where they are
contiguous uint8, or contiguous float32 at a 16-byte aligned address. A captured CNN acting node holds only addresses that live
as long as the handle (no generation to watch beside eval_state_gen). Refused in the constructor: an environment without the
attribute (NotImplementedError), a non-bool value (ValueError), hip_cnn_act=True on an attached engine that is no image engine
with the CNN acting path (NotImplementedError: hip_cnn_act does nothing there, drop it) -- for a policy attached later, at the
first run_evaluation, before an environment or engine call; at the first run_evaluation: an engine off the GPU. A capture that
raises is ended and re-raised as a RuntimeError naming the environment.

Evaluation draws nothing from the torch or NumPy generators and enqueues no update: the training state is not touched.
After run_evaluation, `returns` (float64[E]), `lengths` (int32[E]) and `steps` (lockstep steps made) describe the last run.

Recording the episodes (`eval_save=True` with `save_folder`; default off: exactly the calls above): the
reference's eval_save (training/evaluator.py:26, 40-73) -- every evaluation episode written to
save_folder/evaluator/iter{iteration}_ep{k}.npy as the dict {"reward_list", "action_list", "obs_list"}, one entry per step; load
one with np.load(path, allow_pickle=True).item(). The rows never leave the GPU during the evaluation: dsact_eval_trace_begin
follows dsact_eval_begin, every lockstep step issues ONE more launch (dsact_eval_record, between the clip and env.step: the
observation rows the acting call read and the action the environment receives) and dsact_eval_commit also stores the reward;
after dsact_eval_read the first `hip_eval_save_episodes` episodes (default: all) are read back one by one and written.
reward_list holds Python floats (the float32 rewards, exactly), action_list float32[A] rows, obs_list rows in the shape and dtype
the environment returned (byte frames stay uint8[C, H, W]). k counts the episodes of one `iteration` value from 0 and keeps
counting when run_evaluation is called again with the same value (the reference's print_time, evaluator.py:35-39).
`hip_eval_save_max_steps` (default: the environment's max_episode_steps attribute; required where it has none) is the number of
steps kept per episode: a longer episode's file holds its first steps, `trace_dropped` counts the (row, step) pairs left out and
one RuntimeWarning per evaluation names them; TAR, returns and lengths are not affected. The trace takes
episodes * steps * (observation row + 4 A + 4) bytes of device memory; above `hip_eval_save_max_bytes` (default 1 << 30) the
first run_evaluation refuses, before any call is made. Under hip_graph_eval the record is a node of the captured window.

The reference's environment wrappers (`hip_env_wrap=True`; default off: exactly the calls above): the
constructor puts the environment it resolved through training/hip_tensor_env_wrappers.wrap_tensor_env with `max_episode_steps`,
`reward_shift`, `obs_shift` and `obs_scale` from the flat argument dict (the reference's Evaluator clears reward_scale only, so
the shift stays and returns sum the shifted reward). Refused (ValueError): a non-bool value, and True with none of the four set.
The per-engine set-up hands the engine to an environment that has `bind_engine`; a wrapped environment's `max_episode_steps` is
eval_save's default step bound.

The reference's image pipeline (`hip_frame_pipe=True`; default off): the constructor puts the environment
through training/hip_tensor_frame_pipe.frame_pipe_tensor_env with `frame_gray`, `frame_stack` and `action_repeat` from the flat
argument dict, before hip_env_wrap. The evaluator KEEPS the repeat (the reference's Evaluator drops only the generic repeat_num
wrapper; CarRacing's built-in repeat stays): lengths count outer steps, returns sum the summed rewards, eval_save records the
stacks. Refused (ValueError): a non-bool value, and True with none of the three set.
"""
import os
import warnings

import numpy as np
import torch

from training.hip_acting_common import (EvalEpisodeCounter, engine_stream, eval_save_kwargs, hand_over, image_graph_engine, networks_of,
                                        on_stream, require_graph_cnn_pair, require_graph_device, require_tensor_engine, tensor_limits,
                                        write_eval_episode)
from training.hip_tensor_env_wrappers import env_wrap_kwargs, wrap_tensor_env
from training.hip_tensor_frame_pipe import frame_pipe_kwargs, frame_pipe_tensor_env

__all__ = ["HipTensorEnvEvaluator"]


class HipTensorEnvEvaluator:
    def __init__(self, index=0, **kwargs):
        self.num_eval_episode = int(kwargs.get("num_eval_episode", 5))
        if self.num_eval_episode < 1:
            raise ValueError("num_eval_episode must be >= 1 (got %d)" % self.num_eval_episode)
        # eval_save: refused here, before an environment is made or touched
        self.eval_save, self.save_folder = eval_save_kwargs(kwargs)
        self.save_episodes = kwargs.get("hip_eval_save_episodes")
        self.save_episodes = self.num_eval_episode if self.save_episodes is None else int(self.save_episodes)
        if self.eval_save and not 1 <= self.save_episodes <= self.num_eval_episode:
            raise ValueError("hip_eval_save_episodes must be 1 .. num_eval_episode = %d (got %d)" % (self.num_eval_episode, self.save_episodes))
        self.save_max_bytes = int(kwargs.get("hip_eval_save_max_bytes", 1 << 30))
        self.trace_dropped = 0                  # (row, step) pairs past hip_eval_save_max_steps in the last run_evaluation
        self.saved_files = []                   # the files the last run_evaluation wrote, in episode-index order
        self._episode_counter = EvalEpisodeCounter()
        self._trace_on = False                  # an eval_trace_begin of the running evaluation has been made
        self.poll_steps = int(kwargs.get("hip_eval_poll_steps", 16))
        if self.poll_steps < 1:
            raise ValueError("hip_eval_poll_steps must be >= 1 (got %d)" % self.poll_steps)
        self.max_steps = int(kwargs.get("hip_eval_max_steps", 100000))
        env = kwargs.get("eval_env")
        if env is None:
            env = kwargs.get("env")
        if env is None:
            from plugin import create_env
            env = create_env(**kwargs)
        pipe = frame_pipe_kwargs(kwargs, "hip_tensor_env_evaluator")   # hip_frame_pipe; None: off, the default
        if pipe is not None:
            env = frame_pipe_tensor_env(env, **pipe)                # (inside hip_env_wrap, as the reference's Env sits inside wrapping_env)
        wrap = env_wrap_kwargs(kwargs, "hip_tensor_env_evaluator")   # hip_env_wrap; None: off, the default
        if wrap is not None:
            env = wrap_tensor_env(env, **wrap)
        self.env = env
        self.n_envs = int(env.num_envs)
        if self.n_envs < 1:
            raise ValueError("the environment's num_envs must be >= 1 (got %d)" % self.n_envs)
        self.save_max_steps = kwargs.get("hip_eval_save_max_steps")
        if self.save_max_steps is None and self.eval_save:
            self.save_max_steps = getattr(env, "max_episode_steps", None)
            if self.save_max_steps is None:
                raise ValueError("eval_save=True keeps a fixed number of steps per episode and %s has no max_episode_steps attribute: "
                                 "pass hip_eval_save_max_steps" % type(env).__name__)
        if self.eval_save:
            self.save_max_steps = int(self.save_max_steps)
            if self.save_max_steps < 1:
                raise ValueError("hip_eval_save_max_steps must be >= 1 (got %d)" % self.save_max_steps)
        self.action_type = kwargs.get("action_type", "continu")
        self.cnn_act = bool(kwargs.get("hip_cnn_act", False))   # image environments on an engine with the CNN acting path
        # hip_graph_eval: the poll windows as one captured graph. Refused here, before any environment or
        # engine call
        graph = kwargs.get("hip_graph_eval", False)
        if not isinstance(graph, (bool, np.bool_)):
            raise ValueError("hip_graph_eval must be True or False, got %r" % (graph,))
        self.graph_eval = bool(graph)
        if self.graph_eval and self.cnn_act and kwargs.get("networks") is not None:
            # the pair is for image engines with the CNN acting path; a policy attached later is checked
            # at the first run_evaluation, before anything runs
            require_graph_cnn_pair("hip_graph_eval", kwargs["networks"])
        if self.graph_eval and getattr(env, "capture_safe", False) is not True:
            raise NotImplementedError("hip_graph_eval=True needs an environment with the attribute capture_safe = True (step and "
                                      "reset(mask) update their state tensors in place, allocate nothing that outlives the call, "
                                      "never touch the host and stay on torch's current stream); %s does not promise it"
                                      % type(env).__name__)
        self.graph_captures = 0   # captures made / replays issued (the capturing call makes the first replay)
        self.graph_replays = 0
        self._graph = None        # the captured window of hip_eval_poll_steps steps (torch.cuda.CUDAGraph)
        self._graph_gen = None    # the engine's eval_state_gen it was captured under: the ev_* addresses it holds
        self._graph_windows = 0   # full windows run on this engine: 0 -> eager warm-up, 1 -> capture, later -> replay
        self.steps = 0            # lockstep steps of the last run_evaluation
        self.returns = None       # its episode returns, float64[E] in episode-index order
        self.lengths = None       # its episode lengths, int32[E]
        self._ready = None        # id of the engine the buffers / clip route were set up for
        self.networks = networks_of(kwargs)   # evaluator.py:16-20: the generator is consumed as HipEvaluator's
        if kwargs.get("networks") is not None:
            self._engine()        # an explicit policy is checked right away

    def load_state_dict(self, state_dict):
        self.networks.load_state_dict(state_dict)

    def _engine(self):
        """the engine behind the ATTACHED MLP policy (hip_cnn_act=True: or CNN policy with the CNN acting path); every other
        setup is refused"""
        if self.graph_eval and self.cnn_act:
            require_graph_cnn_pair("hip_graph_eval", self.networks)
        return require_tensor_engine("hip_tensor_env_evaluator", self.networks, self.action_type, self.env, self.cnn_act)

    def _setup(self, eng):
        """once per engine: the [N, .] buffers and whether the policy's limits are the environment's"""
        N, O, A = self.n_envs, eng.obs_dim, eng.act_dim
        dev = torch.device(eng.device)
        if callable(getattr(self.env, "bind_engine", None)):
            self.env.bind_engine(eng)     # a wrapped environment's step / reset as one launch each
        if self.graph_eval:
            require_graph_device("hip_graph_eval", dev)
            self._graph, self._graph_gen, self._graph_windows = None, None, 0   # a new engine: eager, capture, replay again
            if self.cnn_act and image_graph_engine(eng):
                eng.cnn_acting_capture()   # the CNN route's opt-in to capture
        f = dict(dtype=torch.float32, device=dev)
        self._obs, self._act, self._clip = torch.zeros(N, O, **f), torch.zeros(N, A, **f), torch.zeros(N, A, **f)
        if getattr(eng, "conv_type", None):
            self._obs = None      # image rows [N, C, H, W] in the frame's dtype (float32 or uint8 codes): made at the first reset
        self._rew = torch.zeros(N, **f)
        self._term, self._trunc, self._ended = (torch.zeros(N, dtype=torch.bool, device=dev) for _ in range(3))
        self._low, self._high, self._policy_clip = tensor_limits(self.env, eng, N)
        hand_over(eng)
        self._ready = id(eng)

    def _window(self, eng, count):
        """`count` lockstep steps on torch's current stream: the acting call, the clip where the environment's limits are not the
        policy's, env.step, the commit, env.reset(ended) and the observation hand-over. Without hip_graph_eval every step stages
        reward / terminated / truncated and the next observations in the evaluator's own buffers (the calls this class always
        made). With it -- issued eagerly, under capture, and replayed -- the staging copies leave the dependent chain: eval_commit
        reads the environment's own tensors where they are contiguous float32 / bool [N] on the engine's device, the next
        step's acting call reads the reset's result in place where it is contiguous float32 (image rows: contiguous uint8, or
        float32 at a 16-byte aligned address), and self._obs is written once, at the end: the next window (or an eager remainder) starts from a fixed address."""
        N, env, direct = self.n_envs, self.env, self.graph_eval
        obs, act, clip, rew, term, trunc, ended = self._obs, self._act, self._clip, self._rew, self._term, self._trunc, self._ended
        src = obs
        for _ in range(count):
            eng.act_mode_device(src, act)
            if self._policy_clip:
                a = act
            else:
                a = torch.minimum(torch.maximum(act, self._low), self._high, out=clip)
            if self.eval_save:
                eng.eval_record(src, a)   # what the acting call read and what the environment receives (evaluator.py:53-54)
            obs2, r, te, tr = env.step(a)
            if (direct and r.dtype == torch.float32 and te.dtype == torch.bool and tr.dtype == torch.bool
                    and tuple(r.shape) == tuple(te.shape) == tuple(tr.shape) == (N,) and r.device == te.device == tr.device == rew.device
                    and r.is_contiguous() and te.is_contiguous() and tr.is_contiguous()):
                eng.eval_commit(r, te, tr, ended)
            else:
                rew.copy_(r)
                term.copy_(te)
                trunc.copy_(tr)
                eng.eval_commit(rew, term, trunc, ended)
            # the next step's observations: this step's, with every environment that ended restarted on its own (rows
            # without an episode too)
            nxt = env.reset(ended).reshape(obs.shape)
            if direct and nxt.device == obs.device and nxt.is_contiguous() and (
                    (nxt.dtype == torch.float32 and obs.dim() == 2)
                    or (obs.dim() == 4 and nxt.dtype == obs.dtype
                        and (nxt.dtype == torch.uint8 or (nxt.dtype == torch.float32 and nxt.data_ptr() % 16 == 0)))):
                src = nxt     # (image rows: byte frames as they are, float32 frames where the kernel's 16-byte reads are aligned)
            else:
                obs.copy_(nxt)
                src = obs
        if src is not obs:
            obs.copy_(src)

    def _graph_window(self, eng, stream):
        """one full window (hip_eval_poll_steps steps) of a hip_graph_eval evaluator: the first on an engine runs _window eagerly
        (the warm-up: it makes the library's lazy allocations), the second captures it into a graph on the engine's stream -- one
        linear chain -- and replays it, every later one is one replay. A capture that raises is ended and reported; nothing is
        retried."""
        if self._graph_windows == 0:
            self._window(eng, self.poll_steps)
        else:
            if self._graph is None:
                graph = torch.cuda.CUDAGraph()
                gen = eng.debug_get("eval_state_gen")
                try:
                    with torch.cuda.graph(graph, stream=stream, capture_error_mode="relaxed"):   # (its exit ends the capture)
                        self._window(eng, self.poll_steps)
                except Exception as ex:
                    raise RuntimeError("hip_graph_eval: capturing an evaluation window failed with the environment %s (%s: %s). "
                                       "capture_safe = True promises that step and reset(mask) update state in place, never touch "
                                       "the host and stay on torch's current stream; build the evaluator without hip_graph_eval for "
                                       "this environment" % (type(self.env).__name__, type(ex).__name__, ex)) from ex
                self._graph, self._graph_gen = graph, gen
                self.graph_captures += 1
            self._graph.replay()
            self.graph_replays += 1
        self._graph_windows += 1

    def _trace_bytes(self, eng, row_bytes):
        """the device memory of the trace for observation rows of row_bytes bytes; above hip_eval_save_max_bytes: ValueError"""
        per_step = row_bytes + 4 * eng.act_dim + 4
        total = self.save_episodes * self.save_max_steps * per_step
        if total > self.save_max_bytes:
            raise ValueError("eval_save: the trace takes %d episodes x %d steps x %d bytes per step (a %d-byte observation row, "
                             "the action row and the reward) = %d bytes, above hip_eval_save_max_bytes = %d: lower "
                             "hip_eval_save_episodes or hip_eval_save_max_steps, or raise the bound"
                             % (self.save_episodes, self.save_max_steps, per_step, row_bytes, total, self.save_max_bytes))
        return total

    def _trace_begin(self, eng, obs):
        """eval_trace_begin for rows like obs[N, ...] and, under hip_graph_eval, the generation check over the trace's arrays"""
        row_bytes = int(obs[0].numel()) * int(obs.element_size())
        self._trace_bytes(eng, row_bytes)
        eng.eval_trace_begin(self.save_episodes, self.save_max_steps, row_bytes)
        self._trace_on = True
        if self._graph is not None and eng.debug_get("eval_state_gen") != self._graph_gen:
            self._graph, self._graph_gen, self._graph_windows = None, None, 0   # (the trace's arrays were reallocated)

    def _write_trace(self, eng, iteration):
        """the files of the evaluation that has just been read (evaluator.py:63-73): episode e < hip_eval_save_episodes goes to
        iter{iteration}_ep{k0 + e}; every episode of the evaluation counts in k"""
        ks = [self._episode_counter.next(iteration) for _ in range(self.num_eval_episode)]
        obs_dtype = np.uint8 if self._obs.dtype == torch.uint8 else np.float32
        self.saved_files = []
        for e in range(self.save_episodes):
            raw, act, rew = eng.eval_trace_read(e, min(int(self.lengths[e]), self.save_max_steps))
            rows = np.ascontiguousarray(raw).view(obs_dtype).reshape((raw.shape[0],) + self._row_shape)
            self.saved_files.append(write_eval_episode(self.save_folder, iteration, ks[e], [float(x) for x in rew],
                                                       [a.copy() for a in act], [o.copy() for o in rows]))
        self.trace_dropped = int(eng.debug_get("eval_trace_dropped"))   # (behind eval_read's wait: final)
        if self.trace_dropped:
            warnings.warn("eval_save: %d (episode, step) pairs lie past hip_eval_save_max_steps = %d and are not in the files of "
                          "iteration %s (trace_dropped); returns and lengths are complete"
                          % (self.trace_dropped, self.save_max_steps, iteration), RuntimeWarning, stacklevel=3)

    def run_evaluation(self, iteration):
        eng = self._engine()
        if self.eval_save and not getattr(eng, "conv_type", None):
            self._trace_bytes(eng, 4 * eng.obs_dim)   # refused before any call is made (image rows: once their dtype is known)
        if self._ready != id(eng):
            self._setup(eng)
        pol = self.networks.policy
        if hasattr(pol, "parameters"):
            eng.note_torch_writes(pol.parameters())   # (weights written with torch ops since the last call)
        N, E, P, env = self.n_envs, self.num_eval_episode, self.poll_steps, self.env
        obs = self._obs
        self.steps, remaining = 0, E
        stream = engine_stream(eng)
        with on_stream(stream), torch.no_grad():
            eng.eval_begin(N, E)
            if self._graph is not None and eng.debug_get("eval_state_gen") != self._graph_gen:
                # dsact_eval_begin reallocated the bookkeeping's arrays (another evaluator on this engine asked for more rows or
                # episodes): the graph's eval_commit nodes hold the freed addresses. Eager, capture, replay again
                self._graph, self._graph_gen, self._graph_windows = None, None, 0
            self.trace_dropped, self._trace_on = 0, False
            if self.eval_save and obs is not None:
                self._trace_begin(eng, obs)
            first = env.reset()
            if obs is None:
                row = tuple(getattr(eng, "obs_shape", None) or first.shape[1:])
                odt = torch.uint8 if first.dtype == torch.uint8 else torch.float32
                obs = self._obs = torch.zeros((N,) + row, dtype=odt, device=first.device)
            self._row_shape = tuple(first.shape[1:])   # a saved observation row keeps the shape the environment returns
            if self.eval_save and not self._trace_on:
                self._trace_begin(eng, obs)            # (image rows on a new engine: the frames' dtype is known only now)
            obs.copy_(first.reshape(obs.shape))
            # windows of P lockstep steps (the last one shorter where hip_eval_max_steps is no multiple of P), one wait behind each
            while self.steps < self.max_steps:
                count = min(P, self.max_steps - self.steps)
                if self.graph_eval and count == P:
                    self._graph_window(eng, stream)
                else:
                    self._window(eng, count)
                self.steps += count
                remaining = eng.eval_poll()   # (drains the stream: the handle is idle when the error below is raised)
                if remaining == 0:
                    break
            if remaining != 0:
                if self.eval_save:
                    eng.eval_trace_end()
                raise RuntimeError("hip_tensor_env_evaluator: %d of %d episodes have not ended after hip_eval_max_steps = %d lockstep "
                                   "steps" % (remaining, E, self.max_steps))
            self.returns, self.lengths = eng.eval_read(E)
            if self.eval_save:
                try:
                    self._write_trace(eng, iteration)
                finally:
                    eng.eval_trace_end()
        return np.mean(self.returns)   # episode-index order (evaluator.py:77-81)
