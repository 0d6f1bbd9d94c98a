"""The captured-graph bookkeeping behind dsact_run_group / dsact_graph_build (csrc/dsact_api.hip: the active graph, the cache of
inactive ones, the launch forms of the pipelined graph), pinned on three sequences test_hip_groups.py leaves open:

  * one group length in BOTH noise modes (device Philox / the uploaded noise table): two graphs of the same length, swapped
    through the cache on every group;
  * a refused dsact_graph_build between groups: the active graph and the cache stay as they were;
  * every launch form of the pipelined graph's backward in one replay, with the merged backward launches on and off.

Each against the same updates issued eagerly, bit for bit. Smallest shape that takes the pipelined graph."""
import numpy as np
import pytest
import torch

from dsact._ffi import F_SKIP_ACTOR_ON_OFF_ITERS, DsactError
from oracle.dsact_oracle import draw_noise
from test_hip_groups import fill, host_ring, noise_row, same_engine_state
from test_hip_parity import make_pair

pytestmark = pytest.mark.gpu

O, A, HID, B, D, N = 16, 4, (64, 64), 64, 2, 3000
SEED = 4242


def engine(ring):
    alg, _ = make_pair(O, A, HID, B, seed=4, delay_update=D)
    e = alg.engine
    e.set_device_rng(SEED)
    fill(e, ring)
    return e


def index_rows(total, seed):
    np.random.seed(seed)
    return np.stack([np.random.randint(0, N, size=B) for _ in range(total)])


def eager(e, first, rows, noises=None):
    """the updates of one group issued one by one; noises: the reference's draws (set_noise), None: device Philox noise"""
    for j in range(len(rows)):
        if noises is None:
            e.set_device_rng(SEED)          # (set_noise switched the handle to the uploaded noise)
        else:
            z = noises[j]
            e.set_noise(z["eps_new"].numpy(), z["eps_2"].numpy(), z["z5"].numpy(), z["z6"].numpy())
        e.gather(rows[j])
        e.step(first + j)


def test_one_length_in_both_noise_modes_through_the_cache():
    ring = host_ring(N, O, A, 3)
    modes = [True, False, True, False]      # noise table, device RNG, table, RNG: groups of 4
    rows = index_rows(4 * len(modes), 7)
    torch.manual_seed(99)
    noises = [draw_noise(B, A) for _ in range(len(rows))]
    e, g = engine(ring), engine(ring)
    for i, table in enumerate(modes):
        k = 4 * i
        eager(e, k, rows[k:k + 4], noises[k:k + 4] if table else None)
        g.run_group(k, rows[k:k + 4], np.stack([noise_row(z) for z in noises[k:k + 4]]) if table else None)
    e.sync()
    g.sync()
    same_engine_state(e, g, "both noise modes vs eager")
    assert g.debug_get("graph_cache") == 1.0                     # same length, the other noise mode
    assert g.debug_get("graph_noise_table") == (1.0 if modes[-1] else 0.0)
    assert g.debug_get("pipe_graph") == 1.0 and g.debug_get("graph_steps") == 4.0


def test_a_refused_build_leaves_the_graphs_in_place():
    ring = host_ring(N, O, A, 3)
    lengths = [4, 3, 4, 3]
    rows = index_rows(sum(lengths), 7)
    e, g = engine(ring), engine(ring)

    def groups(k, it, some):
        for n in some:
            eager(e, it, rows[k:k + n])
            g.run_group(it, rows[k:k + n])
            k, it = k + n, it + n
        return k, it

    k, it = groups(0, 0, lengths[:2])
    names = ("graph_steps", "pipe_graph", "graph_cache")
    before = [g.debug_get(n) for n in names]
    assert before == [3.0, 1.0, 1.0]
    with pytest.raises(DsactError, match="multiple of delay_update"):
        g.graph_build(3, F_SKIP_ACTOR_ON_OFF_ITERS)              # refused: 3 is no multiple of delay_update
    assert [g.debug_get(n) for n in names] == before
    groups(k, it, lengths[2:])
    e.sync()
    g.sync()
    same_engine_state(e, g, "groups around a refused build vs eager")
    assert [g.debug_get(n) for n in names] == before
    g.graph_build(2)                                             # an explicit build keeps no other graph
    assert g.debug_get("graph_cache") == 0.0 and g.debug_get("graph_steps") == 2.0


@pytest.mark.parametrize("env", [{}, {"DSACT_NO_BQT_MERGE": "1", "DSACT_NO_BQP_MERGE": "1"}], ids=["default", "no_merged_backward"])
def test_every_launch_form_of_the_pipelined_graph_in_one_replay(env, monkeypatch):
    """7 updates from iteration 1 and 2 from iteration 0: updates that leave the policy alone and have a successor (their
    policy backward is deferred), updates that move the policy, and last updates that can neither defer nor precompute --
    with the merged backward launches (k_chain_bwd_qt / k_chain_bwd_qpt) and with the launches they replace."""
    for name in ("DSACT_NO_BQT_MERGE", "DSACT_NO_BQP_MERGE", "DSACT_NO_PIPE_DEFER"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    ring = host_ring(N, O, A, 3)
    rows = index_rows(9, 7)
    e, g = engine(ring), engine(ring)
    for first, lo, hi in ((1, 0, 7), (0, 7, 9)):
        eager(e, first, rows[lo:hi])
        g.run_group(first, rows[lo:hi])
        assert g.debug_get("pipe_graph") == 1.0 and g.debug_get("graph_steps") == float(hi - lo)
    e.sync()
    g.sync()
    same_engine_state(e, g, "launch forms vs eager (%s)" % (sorted(env) or "default"))
    assert g.debug_get("graph_cache") == 1.0
