"""The reference's own `wrapping_env` (utils/wrapping_env.py:77-120: TimeLimit, ShapingRewardData, ScaleObservationData) run on a
NumPy one-row twin of the no-limit episode fixture (tests/envs/synth_tensor_episodes_nolimit.py), recorded for
tests/test_env_wrap_host.py.

    DSACT_REFERENCE_ROOT=<reference checkout> python scripts/env_wrap_golden.py --record
        writes tests/golden/env_wrap.npz: recorded results only -- per row r in ROWS and step s < STEPS the action fed
        ("action" float32[R, STEPS, A]), the observation the step started from ("obs" [R, STEPS, O]), and what the wrapped
        environment returned: "obs2" [R, STEPS, O], "reward" float32[R, STEPS], "done" and "truncated" bool[R, STEPS]
        (info.get("TimeLimit.truncated", False)); an environment that is done restarts before the next step. "obs_scale" is
        the float32 ramp the run used.

gym is not installed where this is recorded: the reference's `from gym.wrappers.time_limit import TimeLimit` resolves to
oracle/ref_loader.py's gym-0.23 stand-in (elapsed += 1; at the limit info["TimeLimit.truncated"] = not done, done = True), the
one the recorded trainer trajectories already rest on. Everything else -- wrapping_env, ShapingRewardData, ScaleObservationData,
ConvertType -- is the reference's own code, run in place.

The twin returns float32 values. Under NumPy 2 the reference's arithmetic on float32 inputs with Python-float parameters stays
float32 (`(r + 0.3) * 0.7`, `(obs + 0.1) * ramp`: one rounded add, one rounded multiply) -- the rule of
training/hip_tensor_env_wrappers.py. With MAX_EPISODE_STEPS = 5 the recording holds episodes that terminate before the limit,
episodes truncated at it, and steps where both fire (truncated stays False); the test asserts all three.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "env_wrap.npz")
ROWS = tuple(range(13))
STEPS = 40
MAX_EPISODE_STEPS = 5
REWARD_SHIFT, REWARD_SCALE, OBS_SHIFT = 0.3, 0.7, 0.1
O, A = 17, 6
for _p in (ROOT, os.path.join(ROOT, "tests", "envs")):
    if _p not in sys.path:
        sys.path.append(_p)


def obs_scale():
    """the per-element scale of the run: a float32 ramp 0.5 .. 1.5 over the row"""
    return np.linspace(0.5, 1.5, O).astype(np.float32)


def action_of(r, s):
    """the action fed to row r at its step s: multiples of 0.1 inside the fixture's limits +-0.4, float32"""
    return (((7 * r + 3 * s + 5 * np.arange(A)) % 9 - 4).astype(np.float32) * np.float32(0.1)).astype(np.float32)


class _Space:
    dtype = np.float32


class NumpyEpisodesRow:
    """SynthTensorEpisodesNoLimit's row r as a gym-0.23 style environment in NumPy: the same integers, the same float32
    operations in the same order; reset() starts the row's next episode (k counts the restarts since the first reset())"""
    observation_space = _Space()
    action_space = _Space()

    def __init__(self, r):
        self.r, self.k, self.t = int(r), -1, 0

    def _obs(self):
        code = (131 * self.r + 71 * self.k + 29 * self.t + 17 * np.arange(O)) % 128
        return code.astype(np.float32) * np.float32(1.0 / 64.0) - np.float32(1.0)

    def reset(self, **kwargs):
        self.k += 1
        self.t = 0
        return self._obs()

    def step(self, action):
        self.t += 1
        a = np.asarray(action, np.float32)
        sq = a[0] * a[0]
        for j in range(1, A):
            sq = sq + a[j] * a[j]
        table = np.float32((37 * self.r + 101 * self.t + 11) % 64) * np.float32(1.0 / 16.0) - np.float32(2.0)
        return self._obs(), np.float32(table - sq), (5 * self.r + 3 * self.k + self.t) % 13 == 0, {}


def run_reference():
    from oracle import ref_loader

    ref_loader.import_reference()
    from utils.wrapping_env import wrapping_env

    ramp = obs_scale()
    out = {"obs_scale": ramp, "action": np.zeros((len(ROWS), STEPS, A), np.float32),
           "obs": np.zeros((len(ROWS), STEPS, O), np.float32), "obs2": np.zeros((len(ROWS), STEPS, O), np.float32),
           "reward": np.zeros((len(ROWS), STEPS), np.float32), "done": np.zeros((len(ROWS), STEPS), bool),
           "truncated": np.zeros((len(ROWS), STEPS), bool)}
    for i, r in enumerate(ROWS):
        env = wrapping_env(NumpyEpisodesRow(r), max_episode_steps=MAX_EPISODE_STEPS, reward_shift=REWARD_SHIFT,
                           reward_scale=REWARD_SCALE, obs_shift=OBS_SHIFT, obs_scale=ramp)
        obs, _ = env.reset()
        for s in range(STEPS):
            act = action_of(r, s)
            obs2, rew, done, info = env.step(act)
            for value in (obs, obs2, rew):
                assert np.asarray(value).dtype == np.float32, np.asarray(value).dtype   # (the float32 rule above)
            out["action"][i, s], out["obs"][i, s], out["obs2"][i, s] = act, obs, obs2
            out["reward"][i, s], out["done"][i, s] = rew, bool(done)
            out["truncated"][i, s] = bool(info.get("TimeLimit.truncated", False))
            obs = env.reset()[0] if done else obs2
    return out


def main(argv):
    if argv != ["--record"]:
        raise SystemExit(__doc__)
    out = run_reference()
    np.savez_compressed(GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes" % (GOLDEN, len(out), os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    main(sys.argv[1:])
