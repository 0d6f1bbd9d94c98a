"""HipVecEvaluator -- the evaluation episodes over N environments in lockstep, all live actions from ONE deterministic
acting call per step (`plugin.create_evaluator(hip_eval_env_num=N, ...)` with N >= 2).

The reference's Evaluator (training/evaluator.py:34-84) -- and HipEvaluator (training/hip_trainer.py) -- plays
`num_eval_episode` episodes one after the other, one module forward + dist.mode() per environment step. Here episode e
(0 .. num_eval_episode - 1) runs on environment e % N, and an environment plays its episodes in index order. Every lockstep
step stacks the observations of the environments that still have an episode running, acts for all of them at once and
steps each of them; an episode ends on `done or info["TimeLimit.truncated"]` (as in HipEvaluator), and an environment with
no episodes left drops out. An episode's return is sum(rewards) in step order, the TAR the np.mean of the returns in
episode-index order: the result does not depend on which environment finishes first, and environment i sees exactly the
resets and actions a HipEvaluator on its own copy would give it for its episodes.

Environment i is `eval_envs[i]`, or `create_env(**kwargs)` seeded with `seed + i` (environment 0 thus gets what
HipEvaluator's environment gets). A container built from `algorithm` consumes the torch generator as HipEvaluator's does.

Acting routes (per step, over the live rows):
  * attached MLP HipStochaPolicy or CNN policy: dsact_act_mode_batch -- the library picks the host forward per row or the
    batched GPU forward from the row count (csrc/dsact_act_batch.h);
  * an unattached container or a shape the library does not serve (act_dim > 32): the module forward over the live batch
    plus create_action_distributions(...).mode().
Evaluation draws nothing from the torch generator and enqueues no update: the training state is not touched.

eval_save=True with save_folder (training/evaluator.py:26, 40-73): episode e of a call is written to
save_folder/evaluator/iter{iteration}_ep{k0 + e}.npy -- k0 the episode counter at the start of the call (the reference's
print_time rule) -- whatever order the episodes finish in, with the dict HipEvaluator writes for that episode on environment
e % N's own copy. The files are written after the loop, in episode-index order.
"""
import numpy as np
import torch

from training.hip_acting_common import (ANY_POLICY, EvalEpisodeCounter, _reset, attached_engine, env_count, eval_save_kwargs, make_envs,
                                        networks_of, write_eval_episode)

__all__ = ["HipVecEvaluator"]


class HipVecEvaluator:
    def __init__(self, index=0, **kwargs):
        self.eval_save, self.save_folder = eval_save_kwargs(kwargs)   # (refused before an environment is made)
        self._episode_counter = EvalEpisodeCounter()
        envs, self.n_envs = env_count(kwargs, "eval_envs", "hip_eval_env_num", noun="evaluation environments")
        self.envs = make_envs(kwargs, envs, self.n_envs)
        self.networks = networks_of(kwargs)   # evaluator.py:16-20: the generator is consumed as HipEvaluator's
        self.num_eval_episode = kwargs.get("num_eval_episode", 5)
        self.action_type = kwargs.get("action_type", "continu")
        self.steps = 0        # lockstep steps of the last run_evaluation
        self.returns = []     # its episode returns, in episode-index order

    def load_state_dict(self, state_dict):
        self.networks.load_state_dict(state_dict)

    def _engine(self):
        """the engine behind an ATTACHED policy that dsact_act_mode_batch serves, else None"""
        eng = attached_engine(self.networks, self.action_type, ANY_POLICY)
        return eng if eng is not None and eng.act_dim <= 32 else None

    def route(self):
        """'engine' | 'module': how the next run_evaluation() acts (see the module docstring)"""
        return "engine" if self._engine() is not None else "module"

    def _act_module(self, obs):
        with torch.no_grad():
            logits = self.networks.policy(torch.from_numpy(obs))
            return self.networks.create_action_distributions(logits).mode().cpu().numpy().reshape(obs.shape[0], -1)

    def run_evaluation(self, iteration):
        E, N, envs = int(self.num_eval_episode), self.n_envs, self.envs
        eng = self._engine()
        if eng is not None:
            eng.note_torch_writes(self.networks.policy.parameters())   # (weights written with torch ops since the last call)
        returns = [None] * E
        episode, rewards, obs = {}, {}, {}
        save = self.eval_save
        ks = [self._episode_counter.next(iteration) for _ in range(E)] if save else None   # episode e -> file k0 + e
        seen, acted, traces = {}, {}, [None] * E   # per live environment: obs_list / action_list; per episode: the three lists

        def begin(i, e):
            episode[i], rewards[i], obs[i] = e, [], _reset(envs[i])[0]
            seen[i], acted[i] = [], []

        for i in range(min(N, E)):
            begin(i, i)
        live = sorted(episode)
        ob = None
        self.steps = 0
        while live:
            m = len(live)
            first = np.asarray(obs[live[0]], dtype=np.float32)
            if ob is None or ob.shape[1:] != first.shape:
                ob = np.empty((N,) + first.shape, np.float32)
            for j, i in enumerate(live):   # the live rows, in environment order
                ob[j] = obs[i]
            rows = ob[:m]
            if eng is not None:
                act = np.empty((m, eng.act_dim), np.float32)
                eng.act_mode_batch_addr(rows.ctypes.data, m, act.ctypes.data)
            else:
                act = self._act_module(rows)
            self.steps += 1
            ended = []
            for j, i in enumerate(live):
                if save:   # evaluator.py:53-54: the observation before the step, the action env.step receives (its own row)
                    seen[i].append(obs[i])
                    acted[i].append(act[j].copy())
                o, r, done, info = envs[i].step(act[j])
                rewards[i].append(r)
                obs[i] = o
                if bool(done) or bool(info.get("TimeLimit.truncated", False)):
                    ended.append(i)
            for i in ended:
                e = episode[i]
                returns[e] = sum(rewards[i])   # the reference's own reduction (evaluator.py:71)
                traces[e] = (rewards[i], acted[i], seen[i])
                if e + N < E:
                    begin(i, e + N)
                else:
                    del episode[i], rewards[i], obs[i]
            if ended:
                live = sorted(episode)
        if save:
            for e in range(E):
                write_eval_episode(self.save_folder, iteration, ks[e], *traces[e])
        self.returns = returns
        return np.mean(returns)   # episode-index order (evaluator.py:74-78)
