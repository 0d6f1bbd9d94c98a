"""Benchmark / test fixture: a BATCHED IMAGE environment that speaks the protocol of training/hip_tensor_sampler.py -- the
dynamics of tests/envs/synth_blob_data.py (a (3, 96, 96) image with a bright square whose horizontal position encodes a target
in [-1, 1]; reward = -(a0 - target)^2 - 0.01 |a|^2; never terminated, truncated after 20 steps) for N environments as rows of
torch tensors on one device, written in torch ops only: it runs on the CPU device as well as on a GPU and never moves a value
to the host.

Environment i is SynthBlob(seed + i) (what make_envs seeds the i-th environment of a lockstep sampler with): its targets are the
draws of np.random.default_rng(seed + i) in SynthBlob's own order -- one uniform(-1, 1) per reset() / step(), each followed by the
3 * 96 * 96 float32 draws of SynthBlob's pixel noise, which are skipped here with PCG64's advance() (13 824 64-bit outputs: a
float32 draw takes half of one). The first DRAWS = 256 draws of every environment are made on the host at construction and
kept on the device; the environment's draw counter indexes them modulo DRAWS (a run of more than 256 resets + steps per
environment repeats its targets; SynthBlob does not).

Pixels: every pixel is a member of BOOK = float32(arange(256) / 255), so a coded ring (hip_obs_codebook) takes the frames:
code = 26 (background, 0.102) or 230 (the square, 0.902; rows 36..59, columns cx - 12 .. cx + 11 as in SynthBlob) plus a noise
code in 0..5 (SynthBlob adds U(0, 0.02) = up to 5.1 / 255) from one of 8 fixed noise planes drawn from torch.Generator(seed),
plane (draw counter + environment index) % 8. `frames="float32"` returns BOOK[code], `frames="uint8"` the code itself: the two
agree through BOOK element for element.

    env.num_envs, env.action_low / env.action_high [A]
    env.reset() -> obs[N, 3, 96, 96]; env.reset(mask[N]) restarts the masked rows and returns every row's current frame
    env.step(clipped[N, A]) -> (obs2[N, 3, 96, 96], reward[N] float32, terminated[N] bool (never set), truncated[N] bool)
    env.state_dict() / env.load_state_dict(sd): the draw counters, episode steps and current frames (CPU tensors)
`env_offset` shifts the environment indices: SynthTensorBlob(1, env_offset=i) is environment i of a larger batch on its own.
"""
import numpy as np
import torch

SHAPE = (3, 96, 96)
DRAWS = 256
PLANES = 8
EPISODE_STEPS = 20
BACKGROUND, SQUARE, NOISE_CODES = 26, 230, 6
BOOK = (np.arange(256) / 255).astype(np.float32)
_NOISE_OUTPUTS = 3 * 96 * 96 // 2     # 64-bit PCG64 outputs behind SynthBlob's rng.random((3, 96, 96), dtype=float32)


def _target_draws(seed, n):
    """(targets float64[n], square centres int64[n]): the first n targets of SynthBlob(seed) and their cx"""
    rng = np.random.default_rng(seed)
    tg = np.empty(n, np.float64)
    for k in range(n):
        tg[k] = float(rng.uniform(-1, 1))
        rng.bit_generator.advance(_NOISE_OUTPUTS)
    cx = np.array([int(round((t + 1) / 2 * 71)) + 12 for t in tg], np.int64)
    return tg, cx


class SynthTensorBlob:
    def __init__(self, num_envs, device="cpu", seed=0, act_dim=3, frames="float32", env_offset=0):
        if frames not in ("float32", "uint8"):
            raise ValueError("frames must be 'float32' or 'uint8' (got %r)" % (frames,))
        self.num_envs, self.device, self.frames = int(num_envs), torch.device(device), frames
        self.seed_value = int(seed or 0)
        N = self.num_envs
        draws = [_target_draws(self.seed_value + int(env_offset) + i, DRAWS) for i in range(N)]
        self.targets = torch.from_numpy(np.stack([d[0] for d in draws]).astype(np.float32)).to(self.device)     # [N, DRAWS]
        self.centres = torch.from_numpy(np.stack([d[1] for d in draws])).to(self.device)                          # [N, DRAWS]
        g = torch.Generator().manual_seed(self.seed_value)
        self.noise = torch.randint(0, NOISE_CODES, (PLANES,) + SHAPE, generator=g, dtype=torch.uint8).to(self.device)
        self.book = torch.from_numpy(BOOK).to(self.device)
        self.action_low = torch.full((act_dim,), -1.0, device=self.device)
        self.action_high = torch.full((act_dim,), 1.0, device=self.device)
        self.index = (torch.arange(N, dtype=torch.int64) + int(env_offset)).to(self.device)
        self.rows = torch.arange(N, dtype=torch.int64, device=self.device)
        self.col = torch.arange(96, dtype=torch.int64, device=self.device)
        self.row_in = ((self.col >= 36) & (self.col < 60))[None, None, :, None]                                  # [1, 1, 96, 1]
        self.draw = torch.zeros(N, dtype=torch.int64, device=self.device)     # draws made so far (the NEXT draw's index)
        self.t = torch.zeros(N, dtype=torch.int64, device=self.device)
        self.target = torch.zeros(N, dtype=torch.float32, device=self.device)
        self.codes = torch.zeros((N,) + SHAPE, dtype=torch.uint8, device=self.device)

    def _draw(self):
        """every row draws its next target: (target[N], the codes of its frame [N, 3, 96, 96])"""
        k = self.draw % DRAWS
        target, cx = self.targets[self.rows, k], self.centres[self.rows, k]
        col_in = (self.col[None, :] >= (cx - 12)[:, None]) & (self.col[None, :] < (cx + 12)[:, None])          # [N, 96]
        square = col_in[:, None, None, :] & self.row_in                                                          # [N, 1, 96, 96]
        base = torch.where(square, SQUARE, BACKGROUND).to(torch.uint8)
        codes = base + self.noise[(self.draw + self.index) % PLANES]
        return target, codes

    def _out(self, codes):
        return codes if self.frames == "uint8" else self.book[codes.to(torch.int64)]

    def reset(self, mask=None):
        if mask is None:
            mask = torch.ones(self.num_envs, dtype=torch.bool, device=self.device)
        target, codes = self._draw()
        self.target = torch.where(mask, target, self.target)
        self.codes = torch.where(mask[:, None, None, None], codes, self.codes)
        self.t = torch.where(mask, torch.zeros_like(self.t), self.t)
        self.draw = self.draw + mask.to(torch.int64)
        return self._out(self.codes)

    def step(self, action):
        reward = -(action[:, 0] - self.target) ** 2 - 0.01 * (action * action).sum(dim=1)
        self.t = self.t + 1
        self.target, self.codes = self._draw()
        self.draw = self.draw + 1
        truncated = self.t >= EPISODE_STEPS
        return self._out(self.codes), reward, torch.zeros_like(truncated), truncated

    def state_dict(self):
        return {"draw": self.draw.cpu().clone(), "t": self.t.cpu().clone(), "target": self.target.cpu().clone(),
                "codes": self.codes.cpu().clone()}

    def load_state_dict(self, sd):
        self.draw, self.t = sd["draw"].to(self.device).clone(), sd["t"].to(self.device).clone()
        self.target, self.codes = sd["target"].to(self.device).clone(), sd["codes"].to(self.device).clone()
