"""Test fixture: SynthTensorEpisodes / SynthTensorEpisodesInplace (tests/envs/synth_tensor_episodes.py, ..._inplace.py) WITHOUT a
time limit of their own -- `limit` is 1 << 30 for every row, so `truncated` is never set and only the arithmetic `terminated`
ends an episode: (5 r + 3 k + t) mod 13 == 0 holds for one t in 1 .. 13, an episode lasts at most 13 steps. The time limit of a
test then comes from the wrapper under test (training/hip_tensor_env_wrappers.py). Observations, rewards
and `terminated` are the parents', bit for bit.

`plan(r, k, M)` is `episode_plan` under an outer limit of M steps, in Python integers: (length, terminated, truncated) with
gym 0.23's rule -- at the limit `truncated` is set only where the episode did not terminate in that very step.
"""
import torch

from synth_tensor_episodes import ACT_LIMIT, A, O, SynthTensorEpisodes  # noqa: F401
from synth_tensor_episodes_inplace import SynthTensorEpisodesInplace

NO_LIMIT = 1 << 30


def free_length(r, k):
    """the step at which environment r's episode number k terminates on its own (1 .. 13)"""
    t = 1
    while (5 * r + 3 * k + t) % 13:
        t += 1
    return t


def plan(r, k, M=None):
    """(length, terminated, truncated) of environment r's episode number k under a wrapper's limit of M steps (None: no limit)"""
    t = free_length(r, k)
    if M is None or t < M:
        return t, True, False
    return M, t == M, t != M


class _NoLimit:
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.limit = torch.full_like(self.limit, NO_LIMIT)


class SynthTensorEpisodesNoLimit(_NoLimit, SynthTensorEpisodes):
    pass


class SynthTensorEpisodesInplaceNoLimit(_NoLimit, SynthTensorEpisodesInplace):
    pass
