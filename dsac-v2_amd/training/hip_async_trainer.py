"""HipOffAsyncTrainer -- HipOffSerialTrainer whose sampler collects the next group's transitions while the device runs the
current group's updates (`plugin.create_trainer(..., trainer="hip_off_async_trainer")`).

Let K = sample_interval and theta_g the policy after every update of the iterations < gK. The serial trainer collects the
transitions S_g with theta_g and then runs group g. This trainer collects S_{g+1} with theta_g -- one group old -- and that
sampler call runs while group g's updates execute:

    iteration gK:           add_batch(S_g); hold the behaviour policy (theta_g: behind everything enqueued so far);
                            issue group g's updates exactly as the serial trainer does
    iteration (g+1)K - 1:   after that iteration's log / evaluation / checkpoint, if (g+1)K < max_iteration:
                            S_{g+1} = sampler.sample() with the held theta_g (added, and its tb dict logged, at (g+1)K)

Every other host-visible operation keeps the serial trainer's order: the sampler's torch.randn draws and environment steps,
the np.random.randint index draws, the strict-RNG noise draws, ring writes, logs, evaluations (which act with the LIVE
weights) and checkpoints. Warm-up and S_0 are unchanged; the total sample count is the serial trainer's; step() called
directly is the serial trainer's (no lag) -- only train() overlaps.

Holding: an engine-backed algorithm holds through its engine (dsact_behaviour_hold: a stream-ordered device copy of the
policy, which dsact_act_sample / dsact_act_sample_batch act with on a stream of their own). The held snapshot of theta_g
completes when group g - 1 completes, so at most two groups are in flight. A plain torch algorithm's sampler gets a
copy.deepcopy of the networks at every hold. Setups in which a held sampler would silently act with the live weights are
refused (NotImplementedError) before anything runs: CNN policies without the CNN acting path, samplers that act through the
module forward, data-parallel handles.

CNN policies: served with `hip_cnn_act=True` in the trainer's kwargs AND an engine whose CNN acting
path is enabled (DsactEngine.cnn_act -- the algorithm was built with the same kwarg); the sampler checks then apply as they
stand, so the sampler needs the kwarg too (without it a CNN policy acts through the module forward, which is refused).
"""
import copy

from training.hip_trainer import HipOffSerialTrainer

__all__ = ["HipOffAsyncTrainer"]


def _engine_of(alg):
    eng = getattr(alg, "engine", None)
    return eng if eng is not None and hasattr(eng, "behaviour_hold") else None


def _check_supported(alg, sampler, kwargs=None):
    eng = _engine_of(alg)
    if sampler is None or eng is None:
        return
    if not hasattr(alg, "hold_behaviour"):
        raise NotImplementedError("hip_off_async_trainer: %s has an engine but no hold_behaviour()" % type(alg).__name__)
    if getattr(eng, "conv_type", None):
        # (the kwarg first: the engine's cnn_act is looked at only when the caller opted in)
        if not (kwargs or {}).get("hip_cnn_act") or not eng.cnn_act:
            raise NotImplementedError("hip_off_async_trainer: CNN policies act through the live weights (the stand-alone CNN forward "
                                      "holds the arena's weight pointers) unless the CNN acting path is enabled: pass "
                                      "hip_cnn_act=True to the algorithm, the sampler and the trainer, or use hip_off_serial_trainer")
    if int(eng.cfg.global_batch) != int(eng.batch) or int(getattr(eng, "comm_world", 1)) > 1:
        raise NotImplementedError("hip_off_async_trainer: data-parallel handles are not supported")
    from training.hip_sampler import HipOffSampler
    from training.hip_vec_sampler import HipVecOffSampler

    if isinstance(sampler, HipVecOffSampler):
        route = sampler.route()
        if route == "module":
            raise NotImplementedError("hip_off_async_trainer: this HipVecOffSampler acts through the module forward (the live "
                                      "weights); a held behaviour policy serves its 'host' and 'gpu' routes only")
        held = route != "single" or sampler.per_row_engine() is eng
    else:
        held = isinstance(sampler, HipOffSampler) and sampler.per_row_engine() is eng
    if not held:
        raise NotImplementedError("hip_off_async_trainer: the sampler does not act through dsact_act_sample (general path, or an "
                                  "unknown sampler class): it would act with the live weights")


class HipOffAsyncTrainer(HipOffSerialTrainer):
    def __init__(self, alg, sampler, buffer, evaluator, **kwargs):
        for k in ("hip_save_run_state", "ini_run_state_dir", "hip_run_state_async"):
            if kwargs.get(k):
                raise NotImplementedError("hip_off_async_trainer: %s is not supported -- between two groups this trainer holds a "
                                          "behaviour policy one group old, state the run-state format does not carry; use "
                                          "hip_off_serial_trainer" % k)
        if sampler is not None:
            sampler.networks = alg.networks   # (what the serial trainer does first: the routes below are those of the learner's nets)
        _check_supported(alg, sampler, kwargs)
        super().__init__(alg, sampler, buffer, evaluator, **kwargs)
        self._engine = _engine_of(alg)

    def _hold(self):
        if self._engine is not None:
            self.alg.hold_behaviour()
        else:
            self.sampler.networks = copy.deepcopy(self.networks)

    def _release(self):
        if self._engine is not None:
            self.alg.release_behaviour()
        else:
            self.sampler.networks = self.networks

    def train(self):
        if self.sampler is None:
            return super().train()
        K = self.sample_interval
        ahead = None          # (samples, sampler_tb) of the next group, collected with the held policy
        self._grouping = True
        try:
            while self.iteration < self.max_iteration:
                it = self.iteration
                sampler_tb = {}
                if it % K == 0:
                    samples, sampler_tb = ahead if ahead is not None else self.sampler.sample()
                    ahead = None
                    self.buffer.add_batch(samples)
                    self._hold()
                alg_tb = self._update(it)
                self._events(alg_tb, sampler_tb)
                if (it + 1) % K == 0 and it + 1 < self.max_iteration:
                    ahead = self.sampler.sample()     # runs while this group's updates execute on the device
                self.iteration += 1
        finally:
            self._grouping = False
            self._release()
        self._finish()
