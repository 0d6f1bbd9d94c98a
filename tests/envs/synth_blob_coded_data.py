"""Test fixture: synth_blob (tests/envs/synth_blob_data.py) with every pixel quantised to the 8-bit CarRacing grid -- the
frame the reference's CarRacing wrapper delivers (`rgb / 255` cast to float32), so every value is an entry of
`CODEBOOK = float32(arange(256) / 255)`. synth_blob's own noise makes its values non-codebook; this stub is for the coded
image ring (hip_obs_codebook)."""
import numpy as np

from synth_blob_data import SynthBlob

CODEBOOK = np.float32(np.arange(256) / 255.0)


class SynthBlobCoded(SynthBlob):
    def _obs(self):
        k = np.clip(np.rint(super()._obs().astype(np.float64) * 255.0), 0, 255).astype(np.int64)
        return CODEBOOK[k]


def env_creator(**kwargs):
    return SynthBlobCoded(seed=kwargs.get("seed", 0) or 0, act_dim=int(kwargs.get("action_dim", 3)))
