"""Test fixture: SynthTensorBlob (tests/envs/synth_tensor_blob.py) with the SAME dynamics, bit for bit and for both `frames`
dtypes, and its state kept in tensors that step / reset(mask) update IN PLACE -- what `capture_safe = True` of the
tensor-environment protocol (training/hip_tensor_sampler.py, DESIGN.md sections 22 and 24) promises: `draw`, `t`, `target` and
`codes` keep their storage for the environment's whole life, nothing that has to outlive a call is allocated in it, no value goes
to the host, and every op runs on torch's current stream. A sample() or an evaluation window of such an environment can be
captured into a graph and replayed.

The parent rebinds the four tensors in every call; a captured graph would go on reading the storage they had at capture time.
With frames="uint8" the returned frames ARE `codes` (the parent returns its state tensor too): a caller reads them before the
next step / reset(mask), in stream order -- the sampler and the evaluator do. state_dict() / load_state_dict() copy into place
as well.
"""
import torch

from synth_tensor_blob import EPISODE_STEPS, SynthTensorBlob


class SynthTensorBlobInplace(SynthTensorBlob):
    capture_safe = True

    def reset(self, mask=None):
        if mask is None:
            mask = torch.ones(self.num_envs, dtype=torch.bool, device=self.device)
        target, codes = self._draw()
        self.target.copy_(torch.where(mask, target, self.target))
        self.codes.copy_(torch.where(mask[:, None, None, None], codes, self.codes))
        self.t.copy_(torch.where(mask, torch.zeros_like(self.t), self.t))
        self.draw.add_(mask.to(torch.int64))
        return self._out(self.codes)

    def step(self, action):
        reward = -(action[:, 0] - self.target) ** 2 - 0.01 * (action * action).sum(dim=1)
        self.t.add_(1)
        target, codes = self._draw()
        self.target.copy_(target)
        self.codes.copy_(codes)
        self.draw.add_(1)
        truncated = self.t >= EPISODE_STEPS
        return self._out(self.codes), reward, torch.zeros_like(truncated), truncated

    def load_state_dict(self, sd):
        self.draw.copy_(sd["draw"].to(self.device))
        self.t.copy_(sd["t"].to(self.device))
        self.target.copy_(sd["target"].to(self.device))
        self.codes.copy_(sd["codes"].to(self.device))
