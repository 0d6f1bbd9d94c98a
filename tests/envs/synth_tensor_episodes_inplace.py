"""Test fixture: SynthTensorEpisodes (tests/envs/synth_tensor_episodes.py) with the SAME dynamics, bit for bit, and its state
kept in tensors that step / reset(mask) update IN PLACE -- what `capture_safe = True` of the tensor-environment protocol
(training/hip_tensor_sampler.py, training/hip_tensor_evaluator.py; DESIGN.md sections 22 and 23) promises: `t` and `k` keep their
storage for the environment's whole life (copy_, add_, zero_), nothing that has to outlive a call is allocated in it (the
returned tensors are temporaries the caller consumes at once), no value goes to the host, and every op runs on torch's current
stream. A poll window of an evaluation of such an environment can be captured into a graph and replayed.

The parent rebinds self.t and self.k to fresh tensors in every call; a captured graph would go on reading the storage they had
at capture time. `episode_plan` and the constants are the parent's.
"""
import torch

from synth_tensor_episodes import ACT_LIMIT, A, O, SynthTensorEpisodes, episode_plan, limit_of  # noqa: F401


class SynthTensorEpisodesInplace(SynthTensorEpisodes):
    capture_safe = True

    def reset(self, mask=None):
        if mask is None:
            self.t.zero_()
            self.k.zero_()
        else:
            self.k.add_(mask.to(torch.int64))
            self.t.copy_(torch.where(mask, torch.zeros_like(self.t), self.t))
        return self._obs()

    def step(self, action):
        self.t.add_(1)
        obs2 = self._obs()
        sq = action[:, 0] * action[:, 0]
        for j in range(1, self.act_dim):
            sq = sq + action[:, j] * action[:, j]
        table = ((37 * self.row + 101 * self.t + 11) % 64).to(torch.float32) * (1.0 / 16.0) - 2.0
        reward = table - sq
        terminated = (5 * self.row + 3 * self.k + self.t) % 13 == 0
        truncated = self.t >= self.limit
        return obs2, reward, terminated, truncated
