"""Test fixture: a BATCHED RGB tensor environment for the frame pipeline (training/hip_tensor_frame_pipe.py; DESIGN.md section
28). It speaks the protocol of training/hip_tensor_sampler.py, is written in torch ops only (CPU and GPU), never moves a value to
the host, and keeps its state in tensors that step / reset(mask) update IN PLACE (`capture_safe = True`), with state_dict() /
load_state_dict().

Row i of an instance is environment r = env_offset + i; it holds t (steps into its episode) and k (episodes it has played since
reset()). Everything is a pure integer function of (r, k, t, pixel):
  * pixel(r, k, t, c, p) = (37 r + 53 k + 71 t + 101 c + 13 p + (p * p) mod 11) mod 256 for colour c and pixel p = y * W + x;
    `layout` "chw" returns [N, 3, H, W], "hwc" [N, H, W, 3] -- RAW values 0..255 as uint8 or float32 (`frames`); "codes"
    returns the c = 0 plane alone as [N, 1, H, W] uint8 codes;
  * step(a): t += 1; terminated = (5 r + 3 k + t) mod 13 == 0 (one t in 1 .. 13, and again every 13 steps: a row that is stepped
    after its end may report another end, which an action repeat must ignore); truncated = t >= limit (default: never);
    reward = table(r, t) + sum_{j >= 1} a_j^2 >= 0, table(r, t) = ((37 r + 101 t + 11) mod 64) / 16 (exact in fp32), the squares
    summed IN ORDER with separate multiplies and adds. a_0 is not used: the reference's CarRacing action map a[0] * 2 - 1 never
    bites, and a non-negative reward keeps its 100-step reward memory silent;
  * reset(mask): rows where the mask is set restart (t = 0, k += 1); every row's current frame is returned.
NumpyRgbRow is row r as a gym-0.21 style NumPy environment (what the reference's CarRacing Env wraps): the same integers, the
same float32 operations in the same order. scripts/frame_pipe_golden.py records the reference on it.
"""
import numpy as np
import torch

A = 3
ACT_LIMIT = 0.4
NO_LIMIT = 1 << 30


def ends_at(r, k):
    """the step at which environment r's episode number k terminates on its own (1 .. 13)"""
    t = 1
    while (5 * r + 3 * k + t) % 13:
        t += 1
    return t


class SynthTensorRgb:
    capture_safe = True

    def __init__(self, num_envs, device="cpu", height=8, width=12, layout="chw", frames="uint8", env_offset=0, limit=NO_LIMIT,
                 act_dim=A, act_limit=ACT_LIMIT):
        if layout not in ("chw", "hwc", "codes") or frames not in ("uint8", "float32"):
            raise ValueError("layout must be 'chw', 'hwc' or 'codes' and frames 'uint8' or 'float32' (got %r, %r)" % (layout, frames))
        if layout == "codes" and frames != "uint8":
            raise ValueError("codes are uint8")
        self.num_envs, self.device = int(num_envs), torch.device(device)
        self.H, self.W, self.layout, self.frames, self.limit = int(height), int(width), layout, frames, int(limit)
        self.act_dim = int(act_dim)
        self.action_low = torch.full((self.act_dim,), -float(act_limit), device=self.device)
        self.action_high = torch.full((self.act_dim,), float(act_limit), device=self.device)
        self.row = (torch.arange(self.num_envs, dtype=torch.int64) + int(env_offset)).to(self.device)
        p = torch.arange(self.H * self.W, dtype=torch.int64, device=self.device)
        plane = 13 * p + (p * p) % 11                                                              # [P]
        C = 1 if layout == "codes" else 3
        c = 101 * torch.arange(C, dtype=torch.int64, device=self.device)
        if layout == "hwc":
            self.base = (plane[:, None] + c[None, :]).reshape(1, self.H, self.W, 3)
        else:
            self.base = (c[:, None] + plane[None, :]).reshape(1, C, self.H, self.W)
        self.t = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
        self.k = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)

    def _frames(self):
        code = ((37 * self.row + 53 * self.k + 71 * self.t)[:, None, None, None] + self.base) % 256
        return code.to(torch.uint8 if self.frames == "uint8" else torch.float32)

    def reset(self, mask=None):
        if mask is None:
            self.t.zero_()
            self.k.zero_()
        else:
            self.k.add_(mask.to(torch.int64))
            self.t.copy_(torch.where(mask, torch.zeros_like(self.t), self.t))
        return self._frames()

    def step(self, action):
        self.t.add_(1)
        sq = torch.zeros(self.num_envs, dtype=torch.float32, device=self.device)
        for j in range(1, self.act_dim):
            sq = sq + action[:, j] * action[:, j]
        table = ((37 * self.row + 101 * self.t + 11) % 64).to(torch.float32) * (1.0 / 16.0)
        terminated = (5 * self.row + 3 * self.k + self.t) % 13 == 0
        return self._frames(), table + sq, terminated, self.t >= self.limit

    def state_dict(self):
        return {"t": self.t.cpu().clone(), "k": self.k.cpu().clone()}

    def load_state_dict(self, sd):
        self.t.copy_(sd["t"].to(self.device))
        self.k.copy_(sd["k"].to(self.device))


def rows_value(r, k, t, shape, dtype):
    """SynthTensorRows' row of environment r in episode k at step t, as a NumPy array: element e (row-major) holds the code
    (37 r + 53 k + 71 t + 13 e + (e * e) mod 11) mod 256 as uint8, or code / 2 - 20 as float32 (exact, both signs)"""
    e = np.arange(int(np.prod(shape)), dtype=np.int64)
    code = ((37 * r + 53 * k + 71 * t + 13 * e + (e * e) % 11) % 256).reshape(shape)
    return code.astype(np.uint8) if dtype == "uint8" else (code.astype(np.float32) * np.float32(0.5) - np.float32(20.0))


class SynthTensorRows(SynthTensorRgb):
    """the same episodes, rewards and flags with rows of ANY shape and dtype ("uint8" / "float32" / "float64"): `rows_value`.
    `calls` counts reset and step calls (a refusal must leave it at 0)."""

    def __init__(self, num_envs, shape, dtype="float32", device="cpu", env_offset=0, limit=NO_LIMIT, act_dim=A, act_limit=ACT_LIMIT):
        super().__init__(num_envs, device=device, env_offset=env_offset, limit=limit, act_dim=act_dim, act_limit=act_limit)
        self.shape, self.dtype, self.calls = tuple(int(s) for s in shape), dtype, 0
        e = torch.arange(int(np.prod(self.shape)), dtype=torch.int64, device=self.device)
        self.base = (13 * e + (e * e) % 11).reshape((1,) + self.shape)

    def _frames(self):
        lead = (37 * self.row + 53 * self.k + 71 * self.t).reshape((-1,) + (1,) * len(self.shape))
        code = (lead + self.base) % 256
        if self.dtype == "uint8":
            return code.to(torch.uint8)
        return (code.to(torch.float32) * 0.5 - 20.0).to(getattr(torch, self.dtype))

    def reset(self, mask=None):
        self.calls += 1
        return super().reset(mask)

    def step(self, action):
        self.calls += 1
        return super().step(action)


class NumpyRgbRow:
    """SynthTensorRgb's row r (layout "hwc", the layout gym renders) as a gym-0.21 style environment in NumPy: reset() -> frame,
    step(a) -> (frame, reward, done, info); reset() starts the row's next episode"""

    def __init__(self, r, height=8, width=12, frames="uint8", limit=NO_LIMIT):
        self.r, self.k, self.t = int(r), -1, 0
        self.H, self.W, self.frames, self.limit = int(height), int(width), frames, int(limit)

    def _frame(self):
        p = np.arange(self.H * self.W, dtype=np.int64)
        code = (37 * self.r + 53 * self.k + 71 * self.t + 101 * np.arange(3)[None, :] + (13 * p + (p * p) % 11)[:, None]) % 256
        return code.reshape(self.H, self.W, 3).astype(np.uint8 if self.frames == "uint8" else np.float32)

    def reset(self, **kwargs):
        self.k += 1
        self.t = 0
        return self._frame()

    def step(self, action):
        self.t += 1
        a = np.asarray(action, np.float32)
        sq = np.float32(0.0)
        for j in range(1, A):
            sq = sq + a[j] * a[j]
        table = np.float32((37 * self.r + 101 * self.t + 11) % 64) * np.float32(1.0 / 16.0)
        done = (5 * self.r + 3 * self.k + self.t) % 13 == 0 or self.t >= self.limit
        return self._frame(), np.float32(table + sq), done, {}
