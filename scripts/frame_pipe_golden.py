"""The reference's own CarRacing pipeline (env_gym/gym_carracing_data.py:23-69: Env.reset, Env.step, Env.rgb2gray -- gray, the
stack of img_stack frames, action_repeat inner steps per action) run on a NumPy one-row twin of the RGB fixture
(tests/envs/synth_tensor_rgb.py NumpyRgbRow), recorded for tests/test_frame_pipe_host.py.

    DSACT_REFERENCE_ROOT=<reference checkout> python scripts/frame_pipe_golden.py --record
        writes tests/golden/frame_pipe.npz: recorded results only -- per row r in ROWS and outer step s < STEPS the action fed
        ("action" float32[R, STEPS, 3]), the stack the step started from ("start" float32[R, STEPS, K, H, W]: the reference's
        float64 stack cast to float32), the stack Env.step returned ("stack", likewise), "reward" float32[R, STEPS], "done"
        bool[R, STEPS] and "ended_at" int32[R, STEPS]: the inner index at which the row ended, -1 where it did not. A row that
        is done restarts through Env.reset() before the next step.

The reference's Env is built with Env.__new__(Env) -- Env.__init__ needs box2d, nothing else does -- with the twin as `self.env`
and `img_stack` / `action_repeat` set. gym is not installed where this is recorded: `import gym` resolves to
oracle/ref_loader.install_stubs()'s stand-in and `from gym.utils import seeding` to an empty module made here.

Asserted while recording: `done == die` at every inner step (the twin's rewards are >= 0, so the 100-step reward memory never
ends an episode; its action map a[0] * 2 - 1 is not seen by the twin's reward), and the summed reward stays float32 (NumPy 2
keeps `0 + np.float32` in float32).

The gray values are the reference's np.dot, whose summation order depends on the BLAS route: the script prints how many recorded
gray elements differ from the sequential float64 rule of training/hip_tensor_frame_pipe.py after the cast to float32; the count
must be within 1e-4 of the elements and no difference above 2**-24 (the test's two conditions).
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_pipe.npz")
ROWS = tuple(range(7))
STEPS = 24
H, W, K, R = 8, 12, 4, 4
for _p in (ROOT, os.path.join(ROOT, "tests", "envs")):
    if _p not in sys.path:
        sys.path.append(_p)


def action_of(r, s):
    """the action fed to row r at its outer step s: multiples of 0.1 inside the fixture's limits +-0.4, float32"""
    return (((7 * r + 3 * s + 5 * np.arange(3)) % 9 - 4).astype(np.float32) * np.float32(0.1)).astype(np.float32)


def sequential_gray(rgb):
    """the rule of training/hip_tensor_frame_pipe.py on an [..., 3] array: float64, every operation rounded on its own"""
    x = rgb.astype(np.float64)
    return ((((x[..., 0] * 0.299 + x[..., 1] * 0.587) + x[..., 2] * 0.114) / 128.0) - 1.0).astype(np.float32)


class _Spy:
    """the twin with every inner step's `die` kept"""

    def __init__(self, env):
        self.env, self.dies, self.frames = env, [], []

    def reset(self):
        frame = self.env.reset()
        self.frames.append(frame)
        return frame

    def step(self, action):
        frame, reward, die, info = self.env.step(action)
        self.dies.append(bool(die))
        self.frames.append(frame)
        return frame, reward, die, info


def run_reference():
    from oracle import ref_loader
    from synth_tensor_rgb import NumpyRgbRow

    if not ref_loader.REFERENCE_ROOT:
        raise SystemExit("set DSACT_REFERENCE_ROOT to a reference checkout")
    ref_loader.install_stubs()
    if "gym.utils.seeding" not in sys.modules:                       # (the module imports the name and never uses it here)
        seeding = types.ModuleType("gym.utils.seeding")
        sys.modules["gym.utils.seeding"] = seeding
        sys.modules["gym.utils"].seeding = seeding
    if ref_loader.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_loader.REFERENCE_ROOT)
    from env_gym.gym_carracing_data import Env

    n = len(ROWS)
    out = {"action": np.zeros((n, STEPS, 3), np.float32), "start": np.zeros((n, STEPS, K, H, W), np.float32),
           "stack": np.zeros((n, STEPS, K, H, W), np.float32), "reward": np.zeros((n, STEPS), np.float32),
           "done": np.zeros((n, STEPS), bool), "ended_at": np.full((n, STEPS), -1, np.int32)}
    grays, rule = [], []
    for i, r in enumerate(ROWS):
        env = Env.__new__(Env)
        env.env = spy = _Spy(NumpyRgbRow(r, H, W))
        env.img_stack, env.action_repeat = K, R
        obs = env.reset()
        for s in range(STEPS):
            act = action_of(r, s)
            spy.dies = []
            obs2, rew, done, _ = env.step(act)
            assert np.asarray(rew).dtype == np.float32, np.asarray(rew).dtype          # (the float32 rule above)
            assert not any(spy.dies[:-1]) and spy.dies[-1] == bool(done) and (done or len(spy.dies) == R), spy.dies   # done == die
            out["action"][i, s], out["start"][i, s], out["stack"][i, s] = act, obs, obs2
            out["reward"][i, s], out["done"][i, s] = rew, bool(done)
            out["ended_at"][i, s] = len(spy.dies) - 1 if done else -1
            obs = env.reset() if done else obs2
        for frame in spy.frames:
            grays.append(np.asarray(Env.rgb2gray(frame)).astype(np.float32))
            rule.append(sequential_gray(frame))
    grays, rule = np.stack(grays), np.stack(rule)
    differ = int((grays.view(np.uint32) != rule.view(np.uint32)).sum())
    worst = float(np.abs(grays.astype(np.float64) - rule.astype(np.float64)).max())
    print("gray: %d of %d recorded elements differ from the sequential rule after the cast (cap %d), max |diff| = %.3g (cap %.3g)"
          % (differ, grays.size, int(1e-4 * grays.size), worst, 2.0 ** -24))
    assert differ <= 1e-4 * grays.size and worst <= 2.0 ** -24
    return out


def main(argv):
    if argv != ["--record"]:
        raise SystemExit(__doc__)
    out = run_reference()
    np.savez_compressed(GOLDEN, **out)
    print("wrote %s: %d arrays, %d bytes" % (GOLDEN, len(out), os.path.getsize(GOLDEN)))
    assert os.path.getsize(GOLDEN) <= 300 * 1024


if __name__ == "__main__":
    main(sys.argv[1:])
