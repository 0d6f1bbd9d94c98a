"""The reference's Evaluator with eval_save=True (training/evaluator.py:26, 40-73), run on the evaluator case of
oracle/reference_vectors.py -- synthetic Pendulum, (32, 32) nets, a 60-step time limit, 3 episodes per evaluation -- with
`algorithm="DSAC_V2_HIP"`: it acts with dsac_v2_hip.ApproxContainer on the CPU, found by its own discovery rule.

    DSACT_REFERENCE_ROOT=<reference checkout> python scripts/eval_save_golden.py --run FOLDER
        writes FOLDER/init.npz (the container's weights after torch.manual_seed(SEED)) and lets the reference write
        FOLDER/evaluator/iter{iteration}_ep{k}.npy for run_evaluation(it), it in ITERATIONS
    DSACT_REFERENCE_ROOT=<reference checkout> python scripts/eval_save_golden.py --record
        the same run, packed into tests/golden/eval_save_reference.npz: recorded results only (the weights, and per file
        the three lists as arrays: "<file>/reward_list" float64[T], "<file>/action_list" float32[T, A], "<file>/obs_list" [T, O])

tests/test_eval_save_host.py compares HipEvaluator's files with the packed lists (always) and with a live --run (where a
reference checkout is named). `pack` is what both sides use to turn a folder of files into arrays.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_save_reference.npz")
SEED = 9
ITERATIONS = (0, 0, 1)          # the same value twice: ep0..ep2, then ep3..ep5; another value: ep0..ep2 again
MAX_EPISODE_STEPS = 60
for _p in (ROOT, os.path.join(ROOT, "dsac-v2_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "envs")):
    if _p not in sys.path:
        sys.path.append(_p)


def case_kwargs(save_folder):
    """oracle/reference_vectors.py's evaluator case with the 60-step limit and eval_save switched on"""
    from helpers import hip_kwargs
    from oracle import reference_vectors as rv

    return dict(rv.evaluator_kwargs(hip_kwargs, save_folder), eval_save=True, max_episode_steps=MAX_EPISODE_STEPS)


def pack(folder):
    """{"<file>/<list>": array} for every iter*_ep*.npy of folder/evaluator, with the element types checked: rewards are
    Python or NumPy floats (kept as float64, which holds either exactly), action and observation rows are arrays of one dtype"""
    out = {}
    d = os.path.join(folder, "evaluator")
    for name in sorted(os.listdir(d)):
        if not name.endswith(".npy"):
            continue
        ep = np.load(os.path.join(d, name), allow_pickle=True).item()
        assert sorted(ep) == ["action_list", "obs_list", "reward_list"], (name, sorted(ep))
        T = len(ep["reward_list"])
        assert T >= 1 and len(ep["action_list"]) == len(ep["obs_list"]) == T, name
        assert all(isinstance(r, (float, np.floating)) for r in ep["reward_list"]), name
        stem = name[:-len(".npy")]
        out[stem + "/reward_list"] = np.array([float(r) for r in ep["reward_list"]], np.float64)
        for key in ("action_list", "obs_list"):
            rows = ep[key]
            assert all(isinstance(r, np.ndarray) and r.dtype == rows[0].dtype and r.shape == rows[0].shape for r in rows), (name, key)
            out[stem + "/" + key] = np.stack(rows)
    return out


def run_reference(folder):
    """the reference's Evaluator on the case, files under folder/evaluator; returns {"init/<key>": weights, "tar": TARs}"""
    from oracle import ref_loader

    ref_loader.import_reference()
    case = case_kwargs(folder)
    import plugin

    plugin.install()
    import training.evaluator as ref_eval_mod

    os.makedirs(os.path.join(folder, "evaluator"), exist_ok=True)   # (the reference expects the directory)
    torch.manual_seed(SEED)
    ev = ref_eval_mod.Evaluator(**dict(case))
    out = {"init/" + k: v.numpy().copy() for k, v in ev.networks.state_dict().items()}
    out["tar"] = np.array([float(ev.run_evaluation(it)) for it in ITERATIONS], np.float64)
    return out


def main(argv):
    if len(argv) == 2 and argv[0] == "--run":
        folder = argv[1]
        os.makedirs(folder, exist_ok=True)
        np.savez(os.path.join(folder, "init.npz"), **run_reference(folder))
    elif argv == ["--record"]:
        import tempfile

        with tempfile.TemporaryDirectory() as folder:
            out = run_reference(folder)
            out.update(pack(folder))
        np.savez_compressed(GOLDEN, **out)
        print("wrote %s: %d arrays, %d bytes" % (GOLDEN, len(out), os.path.getsize(GOLDEN)))
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main(sys.argv[1:])
