"""The Python side of keeping the host-side acting snapshot fresh, on CPU (the GPU side: tests/test_acting_live_weights.py):

  * DataParallelUpdater.__init__ writes the arenas with collectives, past every torch version counter: it calls the
    engine's policy_dirty() once, after the broadcasts (stand-ins without that method are left alone);
  * DsactEngine.note_torch_writes sees slice writes through the arena tensor itself (`engine.online[...]`), which the
    attached parameters (`p.data = view`) do not share a version counter with.
"""
import torch
import torch.distributed as dist

from oracle.dsact_oracle import DsactOracle, default_config
from test_dp_gloo import OracleDPEngine


def _world1(tmp_path):
    if dist.is_initialized():
        return False
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    return True


def test_dp_updater_marks_the_policy_dirty_after_the_broadcast(tmp_path, monkeypatch):
    from dsact.dp import DataParallelUpdater

    calls = []

    class Engine(OracleDPEngine):
        def policy_dirty(self):
            calls.append("policy_dirty")

    real = dist.broadcast
    monkeypatch.setattr(dist, "broadcast", lambda t, *a, **k: (calls.append("broadcast"), real(t, *a, **k))[1])
    created = _world1(tmp_path)
    try:
        torch.manual_seed(0)
        orc = DsactOracle(default_config(11, 3, (32, 32)))
        flat = [t.data for n in DsactOracle.NETS for t in orc.p[n]] + [orc.log_alpha.data]
        DataParallelUpdater(Engine(orc, [], []), broadcast_tensors=flat)
        assert calls == ["broadcast"] * len(flat) + ["policy_dirty"]
        calls.clear()
        DataParallelUpdater(OracleDPEngine(orc, [], []), broadcast_tensors=flat)   # a stand-in without policy_dirty
        assert calls == ["broadcast"] * len(flat)
    finally:
        if created:
            dist.destroy_process_group()


def test_note_torch_writes_sees_arena_slice_writes():
    from dsact.engine import DsactEngine

    class Stub:
        def __init__(self):
            self.online = torch.zeros(64)
            self.dirty = 0

        def policy_dirty(self):
            self.dirty += 1

    s = Stub()
    p = torch.nn.Parameter(torch.zeros(8))
    with torch.no_grad():
        p.data = torch.as_strided(s.online, (8,), (1,), 16)     # as ApproxContainer.attach re-homes a parameter
    DsactEngine.note_torch_writes(s, [p])                     # the first look sets the baseline
    n0 = s.dirty
    DsactEngine.note_torch_writes(s, [p])
    assert s.dirty == n0                                      # nothing written: no refresh
    with torch.no_grad():
        s.online[16:20] += 1.0                                # through the arena tensor: p._version does not move
    assert p._version == 0 and float(p.detach()[0]) == 1.0
    DsactEngine.note_torch_writes(s, [p])
    assert s.dirty == n0 + 1
    DsactEngine.note_torch_writes(s, [p])
    assert s.dirty == n0 + 1
    with torch.no_grad():
        p.add_(1.0)                                           # through the parameter: its own counter
    DsactEngine.note_torch_writes(s, [p])
    assert s.dirty == n0 + 2
