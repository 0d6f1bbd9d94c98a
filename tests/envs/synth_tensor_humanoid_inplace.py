"""Test fixture: SynthTensorHumanoid (tests/envs/synth_tensor_humanoid.py) with the SAME dynamics, bit for bit, and its state
kept in tensors that step / reset(mask) update IN PLACE -- what `capture_safe = True` of the tensor-environment protocol
(training/hip_tensor_sampler.py) promises: `pos` and `t` keep their storage for the environment's whole
life, nothing that has to outlive a call is allocated in it (the returned tensors are temporaries the sampler consumes at
once), no value goes to the host, and every op runs on torch's current stream. A sample() of such an environment can be
captured into a graph and replayed.

The parent rebinds self.pos and self.t to fresh tensors in every call; a captured graph would go on reading the storage they
had at capture time. state_dict() / load_state_dict() (the optional resume methods of the protocol) copy into place as well.
"""
import torch

from synth_tensor_humanoid import POOL, TERMINAL_ABOVE, SynthTensorHumanoid


class SynthTensorHumanoidInplace(SynthTensorHumanoid):
    capture_safe = True

    def reset(self, mask=None):
        if mask is None:
            self.pos.copy_(self.first_pos)
            self.t.zero_()
        else:
            self.pos.copy_(torch.where(mask, (self.pos + 17) % POOL, self.pos))
            self.t.copy_(torch.where(mask, torch.zeros_like(self.t), self.t))
        return self.pool[self.pos]

    def step(self, action):
        self.pos.copy_((self.pos + 1 + (action[:, 0] > 0).to(torch.int64)) % POOL)
        self.t.add_(1)
        obs2 = self.pool[self.pos]
        reward = 0.01 * obs2[:, 0] - (action * action).sum(dim=1)
        terminated = obs2[:, 0] > TERMINAL_ABOVE
        truncated = self.t >= self.episode_limit
        return obs2, reward, terminated, truncated

    def state_dict(self):
        return {"pos": self.pos.cpu().clone(), "t": self.t.cpu().clone()}

    def load_state_dict(self, sd):
        self.pos.copy_(sd["pos"].to(self.device))
        self.t.copy_(sd["t"].to(self.device))
