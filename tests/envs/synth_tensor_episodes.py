"""Test fixture: a BATCHED tensor environment whose episode ends are ARITHMETIC -- a fixed function of (row, episodes the row has
played, episode step), never of the state or the action -- so a test knows every episode's length and kind of end beforehand
(`episode_plan`, plain Python integers) while the rewards still depend on the actions. It speaks the protocol of
training/hip_tensor_sampler.py / training/hip_tensor_evaluator.py, is written in torch ops only (CPU and GPU), and never moves a
value to the host.

Row i of an instance is environment r = env_offset + i; it holds t (steps into its episode) and k (episodes it has played
since reset(): one more per restart through reset(mask)). Nothing depends on how many rows run beside it.
  * obs(r, k, t)[j] = ((131 r + 71 k + 29 t + 17 j) mod 128) / 64 - 1: exact in fp32 on every device;
  * step(a): t += 1; obs2 = obs(r, k, t);
      truncated  = t >= limit(r),              limit(r) = 1 + (7 r + 3) mod 11   (1 .. 11)
      terminated = (5 r + 3 k + t) mod 13 == 0
      reward     = table(r, t) - |a|^2,        table(r, t) = ((37 r + 101 t + 11) mod 64) / 16 - 2 (exact in fp32); |a|^2 is
                   summed over the action dimensions IN ORDER with separate multiplies and adds (the same bits for any N);
  * reset(mask): rows where the mask is set restart (t = 0, k += 1); every row's current observation is returned.
With these constants (checked by tests/test_tensor_evaluator_host.py from `episode_plan` alone): row 0 (limit 4) is truncated at
t = 4 in its episodes k = 0 .. 2, its episode k = 3 ends with BOTH flags set at t = 4, its episode k = 4 is terminated at t = 1
(a length-1 episode, terminated only); row 9 (limit 1) plays episodes of length 1 only. The policy's default limits in the
tests (+-0.4) are the environment's.
"""
import torch

O, A = 17, 6
ACT_LIMIT = 0.4


def limit_of(r):
    return 1 + (7 * r + 3) % 11


def episode_plan(r, k):
    """(length, terminated, truncated) of environment r's episode number k, in Python integers"""
    t = 0
    while True:
        t += 1
        term, trunc = (5 * r + 3 * k + t) % 13 == 0, t >= limit_of(r)
        if term or trunc:
            return t, term, trunc


class SynthTensorEpisodes:
    def __init__(self, num_envs, device="cpu", env_offset=0, obs_dim=O, act_dim=A):
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.action_low = torch.full((self.act_dim,), -ACT_LIMIT, device=self.device)
        self.action_high = torch.full((self.act_dim,), ACT_LIMIT, device=self.device)
        self.row = (torch.arange(self.num_envs, dtype=torch.int64) + int(env_offset)).to(self.device)
        self.limit = 1 + (7 * self.row + 3) % 11
        self.col = torch.arange(self.obs_dim, dtype=torch.int64, device=self.device)
        self.t = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
        self.k = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)

    def _obs(self):
        code = (131 * self.row + 71 * self.k + 29 * self.t)[:, None] + 17 * self.col[None, :]
        return (code % 128).to(torch.float32) * (1.0 / 64.0) - 1.0

    def reset(self, mask=None):
        if mask is None:
            self.t = torch.zeros_like(self.t)
            self.k = torch.zeros_like(self.k)
        else:
            self.k = self.k + mask.to(torch.int64)
            self.t = torch.where(mask, torch.zeros_like(self.t), self.t)
        return self._obs()

    def step(self, action):
        self.t = self.t + 1
        obs2 = self._obs()
        sq = action[:, 0] * action[:, 0]
        for j in range(1, self.act_dim):
            sq = sq + action[:, j] * action[:, j]
        table = ((37 * self.row + 101 * self.t + 11) % 64).to(torch.float32) * (1.0 / 16.0) - 2.0
        reward = table - sq
        terminated = (5 * self.row + 3 * self.k + self.t) % 13 == 0
        truncated = self.t >= self.limit
        return obs2, reward, terminated, truncated
