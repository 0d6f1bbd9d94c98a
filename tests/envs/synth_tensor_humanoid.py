"""Benchmark / test fixture: a BATCHED tensor environment with gym_humanoid's shapes (obs 376, act 17, limits +-0.4) that
speaks the protocol of training/hip_tensor_sampler.py -- N environments as rows of torch tensors on one device, written in
torch ops only (it runs on the CPU device as well as on a GPU, and never moves a value to the host).

Dynamics (deterministic, seeded, and per environment a pure function of (seed, environment index, its own actions): they do
not depend on how many environments run beside it):
  * one pool of 4096 observations drawn from torch.Generator(seed) on the CPU, shared by all environments;
  * environment i holds a pool position p_i (first position: (i * 2654435761 + 97 * seed) mod 4096) and an episode step t_i;
  * step(a): p_i += 1, or 2 when a[i, 0] > 0 (the action moves the state); t_i += 1; obs2 = pool[p_i];
    reward = -|a_i|^2 + 0.01 * obs2[0]; terminated = obs2[0] > 2.25 (state-dependent, about 1.2 % of the pool);
    truncated = t_i >= episode_limit_i (a per-environment limit: an int, or one value per environment);
  * reset(mask): rows where the mask is set restart (t_i = 0, p_i += 17); every row's current observation is returned.
`env_offset` shifts the environment indices: SynthTensorHumanoid(1, env_offset=i) is environment i of a larger batch on its own
(`pool=other.pool` shares the observation pool of an instance with the same seed instead of drawing it again).
"""
import torch

O, A = 376, 17
POOL = 4096
ACT_LIMIT = 0.4
TERMINAL_ABOVE = 2.25


class SynthTensorHumanoid:
    def __init__(self, num_envs, device="cpu", seed=0, episode_limit=1000, env_offset=0, pool=None):
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.seed_value = int(seed or 0)
        if pool is None:      # (`pool`: another instance's pool of the same seed, shared instead of drawn again)
            pool = torch.randn(POOL, O, generator=torch.Generator().manual_seed(self.seed_value))
        self.pool = pool.to(self.device)
        self.action_low = torch.full((A,), -ACT_LIMIT, device=self.device)
        self.action_high = torch.full((A,), ACT_LIMIT, device=self.device)
        idx = torch.arange(self.num_envs, dtype=torch.int64) + int(env_offset)
        self.first_pos = ((idx * 2654435761 + 97 * self.seed_value) % POOL).to(self.device)
        limit = torch.as_tensor(episode_limit, dtype=torch.int64)
        self.episode_limit = (limit.expand(self.num_envs) if limit.ndim == 0 else limit.reshape(self.num_envs)).clone().to(self.device)
        self.pos = self.first_pos.clone()
        self.t = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)

    def reset(self, mask=None):
        if mask is None:
            self.pos = self.first_pos.clone()
            self.t = torch.zeros_like(self.t)
        else:
            self.pos = torch.where(mask, (self.pos + 17) % POOL, self.pos)
            self.t = torch.where(mask, torch.zeros_like(self.t), self.t)
        return self.pool[self.pos]

    def step(self, action):
        self.pos = (self.pos + 1 + (action[:, 0] > 0).to(torch.int64)) % POOL
        self.t = self.t + 1
        obs2 = self.pool[self.pos]
        reward = 0.01 * obs2[:, 0] - (action * action).sum(dim=1)
        terminated = obs2[:, 0] > TERMINAL_ABOVE
        truncated = self.t >= self.episode_limit
        return obs2, reward, terminated, truncated

