"""What the samplers and evaluators share: HipOffSampler, HipVecOffSampler, HipTensorEnvSampler, HipEvaluator, HipVecEvaluator
and HipTensorEnvEvaluator. Plain functions -- constructor steps (each class calls them at its own point: the container build
consumes the torch generator), the question "which engine stands behind this policy", and the tensor-environment setup.
Nothing here runs per environment step.
"""
import contextlib
import os

import numpy as np
import torch

MLP_POLICY = ("HipStochaPolicy",)
ANY_POLICY = ("HipStochaPolicy", "HipCnnStochaPolicy")


def _container(**kwargs):
    """`__import__(algorithm.lower()).ApproxContainer(**kwargs)` -- the reference's rule (off_sampler.py:19-23,
    evaluator.py:16-20): a plain CPU torch module until the learner's attached container replaces it"""
    module = __import__(kwargs["algorithm"].lower())
    return getattr(module, "ApproxContainer")(**kwargs)


def _reset(env):
    out = env.reset()
    if isinstance(out, tuple) and len(out) == 2 and isinstance(out[1], dict):
        return out
    return out, {}


# ---- eval_save: the evaluation episodes on disk -----------------------------------------------------
def eval_save_kwargs(kwargs):
    """(eval_save, save_folder) as the three evaluators take them (training/evaluator.py:25-26): eval_save a bool, default
    False; with it save_folder is required. Refused with ValueError before anything runs and before anything is written."""
    save = kwargs.get("eval_save", False)
    if not isinstance(save, (bool, np.bool_)):
        raise ValueError("eval_save must be True or False, got %r" % (save,))
    folder = kwargs.get("save_folder")
    if save and (folder is None or not isinstance(folder, (str, os.PathLike)) or not str(folder)):
        raise ValueError("eval_save=True writes save_folder/evaluator/iter{iteration}_ep{k}.npy: pass save_folder (got %r)" % (folder,))
    return bool(save), (os.fspath(folder) if save else folder)


class EvalEpisodeCounter:
    """the k of iter{iteration}_ep{k}: the reference's print_time (training/evaluator.py:28-29, 35-39) -- episodes counted from 0
    within one `iteration` value, across run_evaluation calls that pass the same value"""

    def __init__(self):
        self.print_time, self.print_iteration = 0, -1

    def next(self, iteration):
        if self.print_iteration != iteration:
            self.print_iteration, self.print_time = iteration, 0
        else:
            self.print_time += 1
        return self.print_time


def write_eval_episode(save_folder, iteration, k, reward_list, action_list, obs_list):
    """np.save(save_folder/evaluator/iter{iteration}_ep{k}, {"reward_list", "action_list", "obs_list"}) -- training/
    evaluator.py:63-73's dict and file name; the directory is created. Returns the path written (np.save adds .npy)."""
    folder = os.path.join(save_folder, "evaluator")
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, "iter{}_ep{}".format(iteration, k))
    np.save(path, {"reward_list": reward_list, "action_list": action_list, "obs_list": obs_list})
    return path + ".npy"


# ---- constructor steps ------------------------------------------------------------------------------------------------------
def sample_batch_size(kwargs):
    return kwargs["batch_size_per_sampler"] if "batch_size_per_sampler" in kwargs else kwargs["sample_batch_size"]


def explore_noise(kwargs):
    """`noise_params` as the reference's OffSampler reads it for continuous actions (off_sampler.py:32-36: GaussNoise(**noise_params);
    explore_noise.py:17-23: action + np.random.normal(mean, std), before the clip): None, or (mean, std, shared) with mean and std
    the CALLER'S OWN objects -- the host routes hand them to NumPy as they are, so the global generator is consumed exactly as
    the reference consumes it. shared: the draw has shape () or (1,) -- one normal for every action dimension; else it has shape
    (A,): one per dimension (the length is checked against `action_dim` here when the kwargs carry it, and by
    check_noise_dim as soon as a class knows its A). Everything else is refused, before anything runs."""
    params = kwargs.get("noise_params")
    if params is None:
        return None
    if kwargs.get("action_type", "continu") != "continu":
        raise NotImplementedError("exploration noise is served for continuous actions (GaussNoise); the reference's EpsilonGreedy "
                                  "for action_type %r is not part of this path" % (kwargs.get("action_type"),))
    missing = [k for k in ("mean", "std") if k not in params]
    if missing:
        raise NotImplementedError("exploration noise: noise_params needs the keys 'mean' and 'std' of GaussNoise(mean, std); %s "
                                  "missing (EpsilonGreedy's keys are not served)" % " and ".join(repr(k) for k in missing))
    extra = sorted(str(k) for k in params if k not in ("mean", "std"))
    if extra:
        raise ValueError("noise_params takes exactly the keys 'mean' and 'std' (got also %s)" % ", ".join(extra))
    mean, std = params["mean"], params["std"]
    m, s = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    if not np.isfinite(m).all():
        raise ValueError("noise_params['mean'] must be finite (got %r)" % (mean,))
    if not (np.isfinite(s).all() and (s >= 0).all()):
        raise ValueError("noise_params['std'] must be finite and >= 0 (got %r)" % (std,))
    shape = np.broadcast_shapes(m.shape, s.shape)   # np.shape(np.random.normal(mean, std)), without a draw
    if len(shape) > 1:
        raise ValueError("np.random.normal(mean, std) has shape %r: exploration noise is a scalar or one value per action "
                         "dimension" % (shape,))
    noise = (mean, std, shape in ((), (1,)))
    if kwargs.get("action_dim") is not None:
        check_noise_dim(noise, int(kwargs["action_dim"]))
    return noise


def check_noise_dim(noise, act_dim):
    """the shape rule of explore_noise against a known action dimension"""
    if noise is None or noise[2]:
        return
    n = np.broadcast_shapes(np.shape(noise[0]), np.shape(noise[1]))[0]
    if n != act_dim:
        raise ValueError("noise_params: np.random.normal(mean, std) has %d entries, neither 1 nor the action dimension %d"
                         % (n, act_dim))


def noise_shape(noise):
    """np.shape(np.random.normal(mean, std)): (), (1,) or (A,)"""
    return tuple(np.broadcast_shapes(np.shape(noise[0]), np.shape(noise[1])))


def networks_of(kwargs):
    """`networks`, else the reference's own throw-away container (off_sampler.py:19-23, evaluator.py:16-20) -- the trainer replaces
    it with the learner's (trainer.py:24-26), but its random initialisation consumes the torch global generator, so a run from
    the same seed only follows the reference's trajectory if this one is built too"""
    networks = kwargs.get("networks")
    if networks is None and "algorithm" in kwargs:
        networks = _container(**kwargs)
    return networks


def env_count(kwargs, envs_key, count_key, noun="environments"):
    """(kwargs[envs_key] as a list or None, N): N is the list's length, else kwargs[count_key], else 1"""
    envs, n = kwargs.get(envs_key), kwargs.get(count_key)
    if envs is not None:
        envs = list(envs)
        if n is not None and int(n) != len(envs):
            raise ValueError("%s=%s but %d %s were passed" % (count_key, n, len(envs), noun))
        n = len(envs)
    n = int(n) if n is not None else 1
    if n < 1:
        raise ValueError("%s must be >= 1 (got %d)" % (count_key, n))
    return envs, n


def make_envs(kwargs, envs, n):
    """the N environments of a lockstep class from env_count's answer: `envs`, or `create_env(**kwargs)` n times; environment i is
    seeded with `seed + i` (the single-environment classes seed theirs with the plain seed: environment 0 here)"""
    from plugin import create_env

    seed = kwargs.get("seed")
    if envs is None:
        envs = []
        for i in range(n):
            kw_i = dict(kwargs)
            if seed is not None:
                kw_i["seed"] = seed + i
            envs.append(create_env(**kw_i))
    if seed is not None:
        for i, e in enumerate(envs):
            if hasattr(e, "seed"):
                e.seed(seed + i)
    return envs


# ---- the engine behind a policy ---------------------------------------------------------------------------------------------
def attached_engine(networks, action_type, policy_classes):
    """the engine behind an ATTACHED policy of one of `policy_classes` (by class name) that acts continuously, else None. A CNN
    engine counts only where HipCnnStochaPolicy is among the classes."""
    pol = getattr(networks, "policy", None)
    eng = getattr(pol, "_engine", None)
    if eng is None or action_type != "continu" or type(pol).__name__ not in policy_classes:
        return None
    if getattr(eng, "conv_type", None) and "HipCnnStochaPolicy" not in policy_classes:
        return None
    return eng


def cnn_act_engine(networks, action_type):
    """attached_engine for a class that was given `hip_cnn_act=True`: an MLP engine as ever, a CNN engine only with the CNN
    acting path enabled (DsactEngine.cnn_act) -- else None"""
    eng = attached_engine(networks, action_type, ANY_POLICY)
    if eng is not None and getattr(eng, "conv_type", None) and not getattr(eng, "cnn_act", False):
        return None
    return eng


def act_fast_ok(cache, eng):
    """the library's own gate of dsact_act_sample (act_fast_ok, csrc/dsact_api.hip): MLP policy, observation <= 768 floats, at most
    4 hidden layers, act_dim <= 32, DSACT_NO_FAST_ACT unset -- asked once per engine (`cache`: {id(engine): bool}), never restated"""
    ok = cache.get(id(eng))
    if ok is None:
        try:
            ok = eng.debug_get("act_fast") == 1.0
        except Exception:
            ok = False
        cache[id(eng)] = ok
    return ok


# ---- tensor environments (hip_tensor_sampler.py, hip_tensor_evaluator.py) ---------------------------------------------------------
# who -> (what serves the refused setups instead, the library call `who` acts through)
_TENSOR_CLASSES = {"hip_tensor_env_sampler": ("hip_vec_off_sampler", "dsact_act_sample_device"),
                   "hip_tensor_env_evaluator": ("hip_eval_env_num", "dsact_act_mode_device")}


def require_tensor_engine(who, networks, action_type, env, hip_cnn_act=False):
    """the engine behind the ATTACHED MLP policy -- or, for a class that was given `hip_cnn_act=True`, behind a CNN policy whose
    engine has the CNN acting path enabled (DsactEngine.cnn_act; DESIGN.md section 20: the kwarg is read first, the attribute
    only when it is set); every other setup is refused"""
    instead, call = _TENSOR_CLASSES[who]
    pol = getattr(networks, "policy", None)
    eng = getattr(pol, "_engine", None)
    if eng is None:
        raise NotImplementedError("%s needs a policy attached to a DsactEngine (the learner's networks); an "
                                  "unattached container acts through the module forward: use %s" % (who, instead))
    if getattr(eng, "conv_type", None) and not (hip_cnn_act and getattr(eng, "cnn_act", False)):
        raise NotImplementedError("%s serves MLP policies (%s); CNN policies: %s, or hip_cnn_act=True on the algorithm (the "
                                  "engine's CNN acting path) and on %s" % (who, call, instead, who))
    if action_type != "continu":
        raise NotImplementedError("%s serves continuous actions" % who)
    low = torch.as_tensor(env.action_low)
    if low.device != torch.device(eng.device):
        raise ValueError("the environment lives on %s, the engine on %s: %s moves nothing between devices"
                         % (low.device, eng.device, who))
    return eng


def image_graph_engine(eng):
    """an image engine with the CNN acting path (`conv_type` and `cnn_act`): the only engine on which `hip_graph_sample=True` /
    `hip_graph_eval=True` goes together with `hip_cnn_act=True`. Attribute reads only."""
    return bool(getattr(eng, "conv_type", None) and getattr(eng, "cnn_act", False))


def require_graph_cnn_pair(kwarg, networks):
    """`kwarg`=True with hip_cnn_act=True: accepted on an image engine with the CNN acting path, refused on every other ATTACHED
    engine -- there hip_cnn_act does nothing. Reads attributes only (no environment call, no engine method call); an unattached
    policy is left to require_tensor_engine, which refuses it in its own words."""
    eng = getattr(getattr(networks, "policy", None), "_engine", None)
    if eng is not None and not image_graph_engine(eng):
        raise NotImplementedError("%s=True with hip_cnn_act=True needs an image (CNN) policy whose engine has the CNN acting path "
                                  "(hip_cnn_act=True on the algorithm); on this %s engine hip_cnn_act does nothing: drop it"
                                  % (kwarg, "CNN" if getattr(eng, "conv_type", None) else "MLP"))


def require_graph_device(kwarg, dev):
    """a graph is captured from the engine's stream: `kwarg`=True needs an engine on a GPU"""
    if dev.type != "cuda":
        raise NotImplementedError("%s=True needs an engine on a GPU (a graph is captured from its stream); this one is on %s"
                                  % (kwarg, dev))


def tensor_limits(env, eng, n):
    """(low[n, A], high[n, A], same): the environment's action limits as device rows, and whether they are the policy's own
    (dsact_set_action_limits) -- then what the library clips to is what the environment accepts"""
    f = dict(dtype=torch.float32, device=torch.device(eng.device))
    low = torch.as_tensor(env.action_low, **f).expand(n, eng.act_dim).contiguous()
    high = torch.as_tensor(env.action_high, **f).expand(n, eng.act_dim).contiguous()
    e_lo, e_hi = getattr(eng, "act_low", None), getattr(eng, "act_high", None)
    lo_h, hi_h = low.cpu().numpy(), high.cpu().numpy()
    same = bool(e_lo is not None and e_hi is not None and (lo_h == np.asarray(e_lo)[None, :]).all()
                and (hi_h == np.asarray(e_hi)[None, :]).all())
    return low, high, same


def engine_stream(eng):
    """the torch stream the engine's launches go to (None off the GPU)"""
    return getattr(eng, "torch_stream", None) if torch.device(eng.device).type == "cuda" else None


def on_stream(stream):
    """torch ops issued inside are ordered with the engine's launches without any synchronisation"""
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def hand_over(eng):
    """once per engine: buffers, the environment's state and its first observation were produced on torch's current stream; from
    here on everything runs on the engine's. The only wait a tensor-environment class makes on its own."""
    dev = torch.device(eng.device)
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()


def require_env_state(env, who):
    """run_state() / load_run_state() of a sampler carry the environment through two OPTIONAL methods of the environment
    protocol: state_dict() -> a picklable object, load_state_dict(sd) restores it. An environment without them cannot be
    resumed exactly, and that is never promised silently."""
    missing = [m for m in ("state_dict", "load_state_dict") if not callable(getattr(env, m, None))]
    if missing:
        raise NotImplementedError("%s: an exact resume needs the environment's state, but %s offers no %s; add state_dict() "
                                  "(returning a picklable object) and load_state_dict(sd) to it"
                                  % (who, type(env).__name__, " / ".join(m + "()" if m == "state_dict" else m + "(sd)" for m in missing)))
    return env
