"""HipVecOffSampler -- N environments stepped in lockstep, all N actions from ONE batched acting call per step
(`plugin.create_sampler(sampler_name="hip_vec_off_sampler", vector_env_num=N, ...)`).

The reference parses `vector_env_num` / `vector_env_type` and never uses them (example_train/
dsacv2_cnn_carracing_offasync.py:37-38); its OffSampler (training/off_sampler.py:12-101) steps one environment. Here the
per-step host costs -- the acting call, the N(0,1) draw, clipping, the stores -- are paid once per N transitions.

Transitions are STEP-MAJOR: sample() runs S / N lockstep steps (S = batch_size_per_sampler, or sample_batch_size; a
multiple of N), and transition t * N + i is environment i's transition of step t. Replay ring rows and replay indices --
and so a training run's trajectory -- follow this order.

Per environment the semantics are HipOffSampler's (training/hip_sampler.py): the action is clipped to that environment's
action_space, the reward is multiplied by reward_scale, a `TimeLimit.truncated` step is stored as non-terminal, and an
environment that ends (terminal or truncated) is reset on its own while the others go on. Environment i is
`envs[i]`, or `create_env(**kwargs)` seeded with `seed + i` (environment 0 thus gets what HipOffSampler's environment
gets). The throw-away ApproxContainer HipOffSampler builds is built here too, so the torch generator is consumed the same.

Acting routes (per sample(), one per lockstep step):
  * N == 1: HipOffSampler itself -- the run is bitwise HipOffSampler's;
  * attached MLP policy, N >= hip_vec_gpu_min_envs (or hip_vec_act="gpu"): dsact_act_sample_batch, ONE GPU call for the
    N rows with ONE torch.randn(N, A) draw (csrc/dsact_act_batch.h);
  * attached MLP policy below the threshold (or hip_vec_act="host"): dsact_act_sample per row (the host acting forward
    HipOffSampler uses), the N rows of ONE torch.randn(N, A) draw as their eps;
  * hip_cnn_act=True and an attached CNN policy whose engine has the CNN acting path enabled (DsactEngine.cnn_act, DESIGN.md
    section 19): dsact_act_sample_batch on the N frames for every N >= 2. hip_vec_act and hip_vec_gpu_min_envs do not apply:
    a CNN policy has no host forward, so there is nothing to cross over to;
  * other CNN policies and unattached containers: the module forward over the [N, ...] batch plus create_action_distributions
    and its sample() (which consumes the generator as one torch.randn(N, A) draw does).
A row's action depends only on its observation and its eps row: environment i's trajectory does not depend on how many
environments run beside it (given the same draws).

Exploration noise (`noise_params={"mean": ..., "std": ...}`, continuous actions; the reference's GaussNoise, off_sampler.py:58-65
and explore_noise.py:17-23): ONE draw per lockstep step from the global NumPy generator, np.random.normal(mean, std, size=(N,) +
shape) with shape = np.shape(np.random.normal(mean, std)), made right after the step's acting call and before the clip. Row i is
environment i's draw -- bit for bit the i-th of N sequential np.random.normal(mean, std) calls, so N = 1 is HipOffSampler's
trajectory. Row i's action is what `action_i + np.random.normal(mean, std)` gives in NumPy's own arithmetic and dtype (float32
for scalar parameters, whose draw is a Python float; float64 for array parameters); the tuples carry it un-clipped, the clip
and the environment see it, the packed float32 rows get its float32 cast. logp is the un-noised sample's. A shape other than
(), (1,) or (A,), a negative or non-finite std, a non-finite mean or another key: ValueError; a missing key or a discrete
action_type: NotImplementedError -- all before an environment is built.
"""
import time

import numpy as np
import torch

from training.hip_acting_common import (MLP_POLICY, _reset, act_fast_ok, attached_engine, cnn_act_engine, env_count, make_envs,
                                        networks_of, check_noise_dim, explore_noise, noise_shape, sample_batch_size)
from training.hip_sampler import SAMPLER_TIME_KEY, HipOffSampler, SampleBatch

__all__ = ["HipVecOffSampler", "DEFAULT_GPU_MIN_ENVS"]

# the crossover of the batched GPU call and N per-row host calls on the Humanoid policy
DEFAULT_GPU_MIN_ENVS = 32


class HipVecOffSampler:
    def __init__(self, index=0, **kwargs):
        envs, n = env_count(kwargs, "envs", "vector_env_num")
        self.n_envs = n
        self.sample_batch_size = sample_batch_size(kwargs)
        if self.sample_batch_size % n:
            raise ValueError("the sample batch size %d is not a multiple of vector_env_num %d" % (self.sample_batch_size, n))
        self.noise = explore_noise(kwargs)
        self.act_mode = kwargs.get("hip_vec_act", "auto")
        if self.act_mode not in ("auto", "gpu", "host"):
            raise ValueError("hip_vec_act must be 'auto', 'gpu' or 'host' (got %r)" % (self.act_mode,))
        self.gpu_min_envs = int(kwargs.get("hip_vec_gpu_min_envs", DEFAULT_GPU_MIN_ENVS))
        self.cnn_act = bool(kwargs.get("hip_cnn_act", False))   # additive (default False): see the module docstring
        if n == 1:
            # the single-environment sampler as it is: same environment, same container, same per-step calls
            one = dict(kwargs)
            one.pop("envs", None)
            if envs is not None:
                one["env"] = envs[0]
            self._single = HipOffSampler(index, **one)
            return
        self._single = None
        self.envs = envs = make_envs(kwargs, envs, n)
        first = [_reset(e) for e in envs]
        self.obs_shape = np.shape(first[0][0])
        self.obs_dim = int(np.prod(self.obs_shape))
        self.obs = np.empty((n, self.obs_dim), np.float32)
        self.obs[...] = [np.reshape(o, -1) for o, _ in first]
        self.infos = [i for _, i in first]
        self.networks = networks_of(kwargs)   # (the reference's throw-away container: built for its use of the torch generator)
        self.action_type = kwargs.get("action_type", "continu")
        self.reward_scale = kwargs.get("reward_scale", 1)
        self.total_sample_number = 0
        # per-environment action limits as [N, A] rows: the clip is two ufunc calls over the N actions of a step
        self.low = np.stack([np.asarray(e.action_space.low, np.float32).reshape(-1) for e in envs])
        self.high = np.stack([np.asarray(e.action_space.high, np.float32).reshape(-1) for e in envs])
        self._fast_ok = {}
        check_noise_dim(self.noise, self.low.shape[1])

    # HipOffSampler's surface (the trainer assigns `networks`, the evaluator reads the sample count)
    def __getattr__(self, name):
        single = self.__dict__.get("_single")
        if single is not None:
            return getattr(single, name)
        raise AttributeError(name)

    def __setattr__(self, name, value):
        single = self.__dict__.get("_single")
        if single is not None and name != "_single" and not hasattr(type(self), name):   # (a wrapped sample() stays here)
            setattr(single, name, value)
        else:
            object.__setattr__(self, name, value)

    def load_state_dict(self, state_dict):
        self.networks.load_state_dict(state_dict)

    def get_total_sample_number(self):
        return self.total_sample_number

    def _engine(self):
        """the engine behind an ATTACHED MLP policy (dsact_act_sample_batch serves every one) -- with hip_cnn_act also behind a
        CNN policy whose engine has the CNN acting path enabled --, else None"""
        if self.cnn_act:
            return cnn_act_engine(self.networks, self.action_type)
        return attached_engine(self.networks, self.action_type, MLP_POLICY)

    def per_row_engine(self):
        """the engine the 'single' route's per-row dsact_act_sample calls go to (HipOffSampler.per_row_engine of the wrapped
        sampler); None on every other route. What the overlapped trainer asks before it holds the behaviour policy."""
        return self._single.per_row_engine() if self._single is not None else None

    def route(self):
        """'single' | 'gpu' | 'host' | 'module': how the next sample() acts (see the module docstring)"""
        if self._single is not None:
            return "single"
        eng = self._engine()
        if eng is None:
            return "module"
        if getattr(eng, "conv_type", None):
            return "gpu"   # (a CNN policy has no host forward: hip_vec_act / hip_vec_gpu_min_envs do not apply)
        if self.act_mode == "gpu" or (self.act_mode == "auto" and self.n_envs >= self.gpu_min_envs):
            return "gpu"
        return "host" if act_fast_ok(self._fast_ok, eng) else "gpu"

    def sample(self):
        if self._single is not None:
            return self._single.sample()
        t0 = time.perf_counter()
        self.total_sample_number += self.sample_batch_size
        route = self.route()
        N, S, O = self.n_envs, self.sample_batch_size, self.obs_dim
        eng = self._engine() if route in ("gpu", "host") else None
        if eng is not None:
            A = eng.act_dim
            eng.note_torch_writes(self.networks.policy.parameters())   # (weights written with torch ops since the last call)
        else:
            A = self.low.shape[1]
        obs_b, obs2_b = np.empty((S, O), np.float32), np.empty((S, O), np.float32)
        act_b, clip_b = np.empty((S, A), np.float32), np.empty((S, A), np.float32)
        rew_b, done_b, logp_b = np.empty(S, np.float32), np.empty(S, np.float32), np.empty(S, np.float32)
        rew64 = np.empty(N, np.float64)
        eps_t = torch.empty(N, A)
        eps_a = eps_t.data_ptr()
        envs, low, high, scale = self.envs, self.low, self.high, self.reward_scale
        maximum, minimum = np.maximum, np.minimum
        flat = len(self.obs_shape) == 1
        batch = SampleBatch()
        infos = self.infos
        noise = self.noise
        if noise is not None:
            check_noise_dim(noise, A)
            draw_shape = noise_shape(noise)
        obs_b[0:N] = self.obs
        for t in range(S // N):
            r0, r1 = t * N, (t + 1) * N
            ob, ac, lp = obs_b[r0:r1], act_b[r0:r1], logp_b[r0:r1]
            if route == "module":
                obs_t = torch.from_numpy(ob.reshape((N,) + tuple(self.obs_shape)))
                with torch.no_grad():
                    logits = self.networks.policy(obs_t)
                    dist = self.networks.create_action_distributions(logits)
                    action, logp = dist.sample()
                ac[...] = action.detach().cpu().numpy().reshape(N, A)
                lp[...] = logp.detach().cpu().numpy().reshape(N)
            else:
                torch.randn(N, A, out=eps_t)   # ONE draw per lockstep step, row i for environment i
                if route == "gpu":
                    eng.act_sample_batch_addr(ob.ctypes.data, N, eps_a, ac.ctypes.data, lp.ctypes.data)
                else:
                    act_into = eng.act_sample_addr
                    for i in range(N):
                        act_into(ob[i].ctypes.data, eps_a + 4 * A * i, ac[i].ctypes.data, lp[i:i + 1].ctypes.data)
            if noise is not None:
                # ONE draw per lockstep step, row i = the i-th sequential np.random.normal(mean, std); row i's action is
                # `ac[i] + that draw` as NumPy evaluates it (a scalar draw is a Python float there: float32 arithmetic)
                draw = np.random.normal(noise[0], noise[1], size=(N,) + draw_shape)
                ac_t = ac + (draw.astype(np.float32)[:, None] if draw_shape == () else draw)
                ac[...] = ac_t      # (the packed rows: the float32 cast)
                cl = minimum(maximum(ac_t, low), high)
            else:
                ac_t = ac
                cl = clip_b[r0:r1]
                minimum(maximum(ac, low, out=cl), high, out=cl)
            steps = [e.step(cl[i]) for i, e in enumerate(envs)]
            obs2 = obs2_b[r0:r1]
            obs2[...] = [np.reshape(s[0], -1) for s in steps]
            truncs = [bool(s[3].get("TimeLimit.truncated", False)) for s in steps]
            dones = [bool(s[2]) and not tr for s, tr in zip(steps, truncs)]   # time-outs are stored as non-terminal (off_sampler.py:70-73)
            np.multiply(np.asarray([s[1] for s in steps], np.float64), scale, out=rew64)
            rew_b[r0:r1] = rew64
            done_b[r0:r1] = dones
            next_infos = []
            for i, s in enumerate(steps):
                ni = s[3]
                ni["TimeLimit.truncated"] = truncs[i]
                next_infos.append(ni)
                if flat:
                    batch.append((ob[i], infos[i], ac_t[i], float(rew64[i]), obs2[i], dones[i], lp[i], ni))
                else:
                    batch.append((ob[i].reshape(self.obs_shape), infos[i], ac_t[i], float(rew64[i]),
                                  obs2[i].reshape(self.obs_shape), dones[i], lp[i], ni))
            # the next step's observations: this step's, with every environment that ended reset on its own
            nxt = obs_b[r1:r1 + N] if r1 < S else self.obs
            nxt[...] = obs2
            infos = next_infos
            for i, e in enumerate(envs):
                if dones[i] or truncs[i]:
                    o, infos[i] = _reset(e)
                    nxt[i] = np.reshape(o, -1)
        self.infos = infos
        batch.packed = (obs_b, act_b, rew_b, obs2_b, done_b, logp_b)
        return batch, {SAMPLER_TIME_KEY: (time.perf_counter() - t0) * 1000}
