"""The coded image replay ring (`create_buffer(..., hip_obs_codebook=table)`, dsact_buffer_create_coded): obs / obs2 held as
one byte per element, an index into a table of at most 256 float32 values. Stored values come back bit for bit, so the
staged minibatch, every update and every trainer trajectory equal the fp32 ring's for the same transitions and indices.

CPU: the codebook validator (parse_obs_codebook) and its refusals before any engine exists. GPU: gather parity (type_2 and
type_1, wrapping adds), the update flows (eager, graph replay, group, data-parallel world 1, DSAC_V1), the trainer loop, a
ring past 2^31 code bytes, the footprint, and the refusal of values missing from the table."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "dsac-v2_amd")
ENVS = os.path.join(HERE, "envs")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

BOOK = np.float32(np.arange(256) / 255.0)   # CarRacing: the wrapper's rgb / 255 (float64), then the float32 cast


def _kw(obs_shape, A=3, B=8, cap=40, conv_type="type_2", **over):
    from helpers import hip_kwargs

    kw = hip_kwargs(tuple(obs_shape), A, (256, 256, 256), B, act_limit=1.0, buffer_max_size=cap, **over)
    for key in ("value", "policy"):
        kw[key + "_func_type"], kw[key + "_conv_type"] = "CNN", conv_type
        kw.pop(key + "_hidden_sizes")
    return kw


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_validator_accepts_the_carracing_table():
    from training.hip_replay_buffer import parse_obs_codebook

    got = parse_obs_codebook(list(np.arange(256) / 255.0), (3, 96, 96))
    assert got.dtype == np.float32 and got.shape == (256,)
    assert np.array_equal(got.view(np.uint32), BOOK.view(np.uint32))
    assert parse_obs_codebook(BOOK, (4, 84, 84)).dtype == np.float32


@pytest.mark.parametrize("table,match", [
    (np.arange(257) / 256.0, "257 entries"),
    ([0.0, 0.1, 0.1 + 1e-12, 0.5], "not strictly ascending"),   # distinct in float64, a duplicate after the float32 cast
    ([0.0, float("nan"), 1.0], "NaN"),
    ([-0.0, 0.0, 1.0], "not strictly ascending"),
    ([0.0, 0.5, 0.25], "not strictly ascending"),
    ([], "1-D list"),
])
def test_validator_refuses_bad_tables_before_any_engine(table, match, monkeypatch):
    import dsact.engine
    from training import hip_replay_buffer
    from training.hip_replay_buffer import HipReplayBuffer, parse_obs_codebook

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(hip_replay_buffer, "DsactEngine", no_engine)
    monkeypatch.setattr(hip_replay_buffer, "current_engine", no_engine)
    monkeypatch.setattr(dsact.engine, "DsactEngine", no_engine)
    with pytest.raises(ValueError, match="hip_obs_codebook: .*" + match):
        parse_obs_codebook(table, (3, 96, 96))
    with pytest.raises(ValueError, match="hip_obs_codebook"):
        HipReplayBuffer(**_kw((3, 96, 96), hip_obs_codebook=table))


@pytest.mark.parametrize("obsv_dim", [11, (3, 10, 10), (17, 16, 16)])
def test_validator_refuses_flat_and_unsupported_shapes_before_any_engine(obsv_dim, monkeypatch):
    from training import hip_replay_buffer
    from training.hip_replay_buffer import HipReplayBuffer

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(hip_replay_buffer, "DsactEngine", no_engine)
    monkeypatch.setattr(hip_replay_buffer, "current_engine", no_engine)
    kw = dict(obsv_dim=obsv_dim, action_dim=3, buffer_max_size=10, replay_batch_size=4, hip_obs_codebook=BOOK)
    with pytest.raises(NotImplementedError, match="hip_obs_codebook"):
        HipReplayBuffer(**kw)


def test_coded_symbols_are_declared_and_bound():
    from dsact import _ffi

    names = {n for n, _, _ in _ffi.SYMBOLS}
    assert {"dsact_buffer_create_coded", "dsact_buffer_check", "dsact_buffer_bytes"} <= names
    hdr = open(os.path.join(ROOT, "include", "dsact.h")).read()
    for n in ("dsact_buffer_create_coded", "dsact_buffer_check", "dsact_buffer_bytes"):
        assert n + "(" in hdr, n


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _samples(rng, n, obs_shape, A):
    """codebook-valued image transitions as HipReplayBuffer.add_batch takes them"""
    out = []
    for _ in range(n):
        out.append((BOOK[rng.integers(0, 256, obs_shape)], {}, rng.uniform(-1, 1, A).astype(np.float32), float(rng.standard_normal()),
                    BOOK[rng.integers(0, 256, obs_shape)], bool(rng.random() < 0.3), np.float32(rng.standard_normal()), {}))
    return out


def _alg_and_buffer(coded, obs_shape=(3, 96, 96), A=3, B=16, cap=48, conv_type="type_2", seed=0, algo="DSAC_V2_HIP", **over):
    import torch

    if algo == "DSAC_V1_HIP":
        from dsac_v1_hip import DSAC_V1_HIP as Alg
        over = dict(over, algorithm="DSAC_V1_HIP", TD_bound=10, bound=True)
    else:
        from dsac_v2_hip import DSAC_V2_HIP as Alg
    from training.hip_replay_buffer import HipReplayBuffer

    kw = _kw(obs_shape, A, B, cap, conv_type, strict_rng=True, **over)
    torch.manual_seed(seed)
    alg = Alg(**kw)
    buf = HipReplayBuffer(**dict(kw, hip_obs_codebook=BOOK if coded else None))
    assert buf.engine is alg.engine
    assert (buf.codebook is not None) == coded
    return alg, buf


def _state(alg):
    e = alg.engine
    e.sync()
    return {n: getattr(e, n).clone() for n in ("online", "target", "adam_m", "adam_v")}, e.get_state()


def _assert_same_state(a, b):
    import torch

    for n in a[0]:
        assert torch.equal(a[0][n], b[0][n]), n
    assert a[1] == b[1]


@pytest.mark.gpu
@pytest.mark.parametrize("obs_shape,conv_type", [((3, 96, 96), "type_2"), ((4, 84, 84), "type_1")])
def test_gather_parity_with_the_fp32_ring(obs_shape, conv_type):
    """the same adds (wrapping, one with n > capacity) into an fp32 and a coded ring: same size / ptr, and the staged
    minibatch of the same indices is bitwise equal (and equal to the rows that were added)"""
    rng = np.random.default_rng(1)
    rows = _samples(rng, 90, obs_shape, 3)
    out = []
    for coded in (False, True):
        alg, buf = _alg_and_buffer(coded, obs_shape, B=8, cap=40, conv_type=conv_type)
        states = []
        for lo, hi in ((0, 25), (25, 37), (37, 90)):    # wraps; the last add has 53 rows > capacity 40
            buf.add_batch(rows[lo:hi])
            states.append((buf.size, buf.ptr))
        batches = []
        for s in (4, 5):
            np.random.seed(s)
            buf.sample_batch(8)
            batches.append(buf.engine.read_batch())
        buf.check()
        out.append((states, batches))
    assert out[0][0] == out[1][0] == [(25, 25), (37, 37), (40, 10)]
    ring = {}
    for i, s in enumerate(rows):   # sequential store(): the last row written to a slot is what it holds
        ring[i % 40] = s
    for s, (b32, bcode) in zip((4, 5), zip(out[0][1], out[1][1])):
        for k in ("obs", "obs2", "act", "rew", "done", "logp"):
            assert np.array_equal(b32[k].view(np.uint32), bcode[k].view(np.uint32)), (s, k)
        np.random.seed(s)
        idx = np.random.randint(0, 40, size=8)
        for r, i in enumerate(idx):
            want = ring[int(i)]
            assert np.array_equal(bcode["obs"][r].view(np.uint32), want[0].view(np.uint32))
            assert np.array_equal(bcode["obs2"][r].view(np.uint32), want[4].view(np.uint32))


def _tb(tb):
    return [float(tb[k]) for k in list(tb.keys()) if not k.startswith("Time/")]


def _run_flow(flow, coded, algo="DSAC_V2_HIP"):
    import torch

    B, N = 16, 48
    alg, buf = _alg_and_buffer(coded, B=B, cap=N, seed=3, algo=algo)
    e = alg.engine
    buf.add_batch(_samples(np.random.default_rng(7), N, (3, 96, 96), 3))
    np.random.seed(11)
    tbs = []
    if flow == "local_update":
        for it in range(3):
            torch.manual_seed(100 + it)
            tbs.append(_tb(alg.local_update(buf.sample_batch(B), it)))
    elif flow == "graph":
        e.set_device_rng(4242)
        e.upload_index_table(np.random.randint(0, N, size=(4, B)))
        e.graph_build(2)
        e.graph_run(0, 4)
    elif flow == "group":
        torch.manual_seed(5)
        tb = alg.local_update_group(buf.sample_batches(B, 4), 0)
        tbs.append(_tb(tb))
    elif flow == "dp":
        import torch.distributed as dist
        from dsact.dp import DataParallelUpdater

        e.set_device_rng(4242)
        e.upload_index_table(np.random.randint(0, N, size=(4, B)))
        dp = DataParallelUpdater(e, broadcast_tensors=(e.online, e.target, e.adam_m, e.adam_v), overlap=False)
        dp.force_collective = True
        assert dist.is_initialized()
        e.dp_begin(0)
        for _ in range(3):
            dp.step()
        torch.cuda.synchronize()
    buf.check()
    return _state(alg), tbs


@pytest.fixture(scope="module")
def gloo_world1():
    import torch.distributed as dist

    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        dist.init_process_group("gloo", rank=0, world_size=1)
        created = True
    yield
    if created:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("flow,algo", [("local_update", "DSAC_V2_HIP"), ("graph", "DSAC_V2_HIP"), ("group", "DSAC_V2_HIP"),
                                       ("dp", "DSAC_V2_HIP"), ("local_update", "DSAC_V1_HIP")])
def test_updates_equal_the_fp32_ring(flow, algo, gloo_world1):
    """CNN updates at B = 16 reading the coded ring == the same updates reading the fp32 ring: parameters, targets, Adam
    moments and step state bit for bit (eager local_update, a graph replay, local_update_group, the world-1 data-parallel
    step, and DSAC_V1 with CNN nets)"""
    a = _run_flow(flow, False, algo)
    b = _run_flow(flow, True, algo)
    _assert_same_state(a[0], b[0])
    assert a[1] == b[1]


@pytest.mark.gpu
def test_coded_update_against_the_cnn_oracle():
    """one update on a minibatch gathered from the coded ring against DsactCnnOracle on the same rows: tb_info at the gates
    of tests/test_hip_cnn_parity.py (1e-4 absolute, critic loss 1e-5 relative)"""
    import torch
    from oracle.dsact_oracle import TB_KEYS, draw_noise
    from oracle.dsact_oracle_cnn import DsactCnnOracle, cnn_config

    B, A = 16, 3
    alg, buf = _alg_and_buffer(True, B=B, cap=48, seed=4)
    buf.add_batch(_samples(np.random.default_rng(8), 48, (3, 96, 96), A))
    cfg = cnn_config((3, 96, 96), A, "type_2")
    orc = DsactCnnOracle(cfg, state_dict={k: v.cpu() for k, v in alg.networks.state_dict().items()})
    np.random.seed(12)
    batch = buf.sample_batch(B)
    data = {k: batch[k].cpu().clone() for k in ("obs", "act", "rew", "obs2", "done")}
    torch.manual_seed(300)
    noise = draw_noise(B, A)
    torch.manual_seed(300)
    tb = alg.local_update(batch, 0)
    ref = orc.local_update(data, noise, 0)
    for i, k in enumerate(TB_KEYS[:-1]):
        g, w = float(tb[k]), float(ref[k])
        tol = 1e-5 * abs(w) + 1e-6 if i == 7 else 1e-4
        assert abs(g - w) <= tol, (k, g, w)


@pytest.mark.gpu
def test_trainer_loop_equals_the_fp32_ring(tmp_path):
    """HipOffSerialTrainer at sample_interval 8 on a codebook-valued image env: the whole loop (indices, ring states, every
    update's statistics, evaluations, logged scalars) is identical with the fp32 and the coded ring"""
    import json

    for p in (PKG, ENVS):
        if p not in sys.path:
            sys.path.append(p)
    import plugin
    from oracle.trainer_trajectory import TIME_TAGS
    from synth_blob_coded_data import CODEBOOK
    from test_trainer_trajectory import RAM_TAG, derived_kwargs, run_hip_loop

    assert np.array_equal(CODEBOOK.view(np.uint32), BOOK.view(np.uint32))
    case = json.load(open(os.path.join(HERE, "golden", "trainer_trajectory_cnn_si8.json")))["case"]
    case = dict(case, env_id="synth_blob_coded", algorithm="DSAC_V2_HIP", buffer_name="hip_replay_buffer")
    runs = []
    for coded in (False, True):
        d = tmp_path / ("coded" if coded else "fp32")
        kw = derived_kwargs(case, str(d), strict_rng=True)
        if coded:
            kw["hip_obs_codebook"] = BOOK
        alg = plugin.create_alg(**kw)
        buffer = plugin.create_buffer(**kw)
        assert buffer.engine is alg.engine and (buffer.codebook is not None) == coded
        got = run_hip_loop(kw, alg, buffer)
        buffer.check()
        got["scalars"] = [s for s in got["scalars"] if s[0] not in TIME_TAGS and s[0] != RAM_TAG]
        runs.append(got)
    assert any(n == 8 for _, n in runs[1]["groups"])
    for k in ("indices", "buffer", "tb_info", "evals", "scalars", "groups", "samples", "apprfunc_dir"):
        assert runs[0][k] == runs[1][k], k


@pytest.mark.gpu
def test_ring_past_2_31_code_bytes():
    """~80k CarRacing rows filled on the device: the obs code column passes 2^31 bytes at row 77,673; rows on both sides of
    the boundary (and the obs2 column, which starts past it) gather back exactly"""
    import torch
    from dsact.engine import DsactEngine

    shape, A, B, cap = (3, 96, 96), 3, 8, 80_000
    O = int(np.prod(shape))
    e = DsactEngine(shape, A, [256, 256, 256], B, conv_type="type_2")
    e.buffer_create(cap, codebook=BOOK)
    assert e.buffer_bytes == cap * (2 * O + 4 * (A + 3))
    book = torch.as_tensor(BOOK, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    chunk, kept = 8_000, {}
    for row0 in range(0, cap, chunk):
        c0 = torch.randint(0, 256, (chunk * O,), device="cuda", generator=g, dtype=torch.int32)
        c2 = torch.randint(0, 256, (chunk * O,), device="cuda", generator=g, dtype=torch.int32)
        obs, obs2 = book.index_select(0, c0).view(chunk, O), book.index_select(0, c2).view(chunk, O)
        del c0, c2
        act = torch.rand(chunk, A, device="cuda", generator=g)
        rew, done = torch.randn(chunk, device="cuda", generator=g), torch.zeros(chunk, device="cuda")
        e.buffer_fill_device(row0, obs, act, rew, obs2, done)
        for r in (0, 1, 77_671, 77_672, 77_673, 77_674, 79_998, 79_999):
            if row0 <= r < row0 + chunk:
                kept[r] = (obs[r - row0].cpu().numpy(), obs2[r - row0].cpu().numpy(), act[r - row0].cpu().numpy())
        del obs, obs2
    assert e.buffer_size == cap
    e.buffer_check()
    assert 77_673 * O > 2**31 > 77_672 * O
    idx = np.array(sorted(kept), np.int64)
    e.gather(idx)
    got = e.read_batch(with_logp=False)
    for r, i in enumerate(idx):
        o, o2, a = kept[int(i)]
        assert np.array_equal(got["obs"][r].reshape(-1).view(np.uint32), o.view(np.uint32)), i
        assert np.array_equal(got["obs2"][r].reshape(-1).view(np.uint32), o2.view(np.uint32)), i
        assert np.array_equal(got["act"][r], a), i
    e.close()
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_footprint_and_ram_report():
    """dsact_buffer_bytes: cap * (2*O + 4*(A+3)) coded, cap * 4*(2*O + A + 3) fp32; __get_RAM__ reports the same row size"""
    O, A, cap = 3 * 96 * 96, 3, 48
    for coded in (False, True):
        alg, buf = _alg_and_buffer(coded, B=8, cap=cap)
        want = cap * (2 * O + 4 * (A + 3)) if coded else cap * 4 * (2 * O + A + 3)
        assert buf.engine.buffer_bytes == want
        buf.add_batch(_samples(np.random.default_rng(2), 20, (3, 96, 96), A))
        assert buf.__get_RAM__() == pytest.approx(want / cap * 20 / 1e6, rel=0, abs=1e-12)


@pytest.mark.gpu
def test_values_missing_from_the_table_are_refused():
    """a value outside the table is never rounded silently: dsact_buffer_check names it and its ring row, and after the write
    has completed every later call on the handle (here a gather) fails too"""
    from dsact._ffi import DsactError

    alg, buf = _alg_and_buffer(True, B=8, cap=40)
    rows = _samples(np.random.default_rng(5), 12, (3, 96, 96), 3)
    buf.add_batch(rows[:5])
    buf.check()
    bad = rows[5]
    img = bad[4].copy()
    img[1, 7, 9] = 0.5                   # 127.5 / 255: not on the grid
    buf.add_batch([bad[:4] + (img,) + bad[5:]] + rows[6:])
    with pytest.raises(DsactError, match=r"E_INVALID.*hip_obs_codebook.*first recorded: 0\.5 .*ring row 5"):
        buf.check()
    alg.engine.sync()
    np.random.seed(0)
    with pytest.raises(DsactError, match="not in the codebook"):
        buf.sample_batch(8)
    # -0.0 is refused when only 0.0 is in the table (bit equality), on a fresh ring
    alg2, buf2 = _alg_and_buffer(True, B=8, cap=40)
    img = rows[0][0].copy()
    img[0, 0, 0] = -0.0
    buf2.add_batch([(img,) + rows[0][1:]])
    with pytest.raises(DsactError, match=r"-0 \(bits 0x80000000\) at ring row 0"):
        buf2.check()
