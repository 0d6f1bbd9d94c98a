#!/usr/bin/env python3
"""Per-class timeline of the weight-gradient tiles of the merged backward launches (k_chain_bwd_qt, k_chain_bwd_qpt) at the
headline shape (Humanoid 3x256, batch 256, pipelined graph). Needs a library built with -DDSACT_TIMELINE:
    python scripts/build_variant.py tl -DDSACT_TIMELINE
    DSACT_LIB_PATH=$PWD/build/libdsact_tl.so python scripts/tile_tail_classes.py OUT.txt
A tile stamps (csrc/dsact_chain.h) slot 11: kind | bias tile << 8 | ragged quad in the tile << 9 | XCD << 12 | problem << 16,
slot 13: wait ended, slots 14 / 15: begin / end -- the last three on the chip-wide 100 MHz counter. Instrumentation, not a
timed comparison: the stamps cost the tiles a few stores."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dsac-v2_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import torch

O, A, HID, B, N = 376, 17, (256, 256, 256), 256, 100_000


def run(stage):
    os.environ["DSACT_TIMELINE_STAGE"] = stage   # read when the engine is created
    from dsac_v2_hip import DSAC_V2_HIP

    torch.manual_seed(0)
    alg = DSAC_V2_HIP(
        algorithm="DSAC_V2_HIP", obsv_dim=O, action_dim=A, action_type="continu", value_func_type="MLP", policy_func_type="MLP",
        value_hidden_sizes=list(HID), policy_hidden_sizes=list(HID), value_hidden_activation="gelu",
        policy_hidden_activation="gelu", value_output_activation="linear", policy_output_activation="linear",
        policy_act_distribution="TanhGaussDistribution", policy_min_log_std=-20, policy_max_log_std=0.5,
        value_learning_rate=1e-4, policy_learning_rate=1e-4, alpha_learning_rate=3e-4, gamma=0.99, tau=0.005, auto_alpha=True,
        alpha=0.2, delay_update=2, cnn_shared=False, replay_batch_size=B, seed=1, hip_device=0, hip_pad_widths=True,
        action_high_limit=np.full((A,), 0.4, np.float32), action_low_limit=np.full((A,), -0.4, np.float32))
    e = alg.engine
    e.set_device_rng(1)
    e.buffer_create(N)
    g = torch.Generator(device=e.device).manual_seed(1)
    e.buffer_fill_device(0, torch.randn(N, O, device=e.device, generator=g), torch.rand(N, A, device=e.device, generator=g) * 0.8 - 0.4,
                         torch.randn(N, device=e.device, generator=g), torch.randn(N, O, device=e.device, generator=g),
                         (torch.rand(N, device=e.device, generator=g) < 0.01).float())
    np.random.seed(1)
    e.upload_index_table(np.random.randint(0, N, size=(64, B)))
    e.graph_build(8)
    assert e.debug_get("pipe_graph") == 1.0
    e.graph_run(0, 408)   # the stamps of the LAST launch of the stage stay
    e.sync()
    tl = e.debug_read("timeline").view(np.int64).reshape(-1, 16)
    assert e.debug_get("handoff_failures") == 0.0
    e.close()
    return tl


def report(stage, tl, out):
    L = len(HID)
    tl = tl[(tl[:, 14] != 0) & (tl[:, 15] != 0)]
    # the last launch only: begun within 60 us of its end (the stage runs again two updates, ~100 us, earlier, and a block
    # index that does not stamp in every launch -- the riders' count differs between them -- keeps that launch's values)
    stamped = tl[tl[:, 14] > tl[:, 15].max() - 6000]
    t00 = stamped[:, 14].min()
    kind = stamped[:, 11] & 0xff
    tiles = stamped[(stamped[:, 13] != 0) & (kind >= 10) & (kind < 10 + L + 1)]
    out.append("%s: %d workgroups stamped, %d of them tiles; launch span (first begin -> last end) %.2f us"
               % (stage, len(stamped), len(tiles), (stamped[:, 15].max() - t00) / 100.0))

    def label(v):
        pi = int(v >> 16) & 0xff
        net, l = pi // (L + 1), pi % (L + 1)
        name = ("q1", "q2", "pi")[net] if net < 3 else "net%d" % net
        return "%s.%s%s%s" % (name, "out" if l == L else "l%d" % l, " +bias" if v & 0x100 else "", " +ragged" if v & 0x200 else "")

    labels = np.array([label(int(v)) for v in tiles[:, 11]])
    after = (tiles[:, 15] - tiles[:, 13]) / 100.0
    end = (tiles[:, 15] - t00) / 100.0
    wait_end = (tiles[:, 13] - t00) / 100.0
    out.append("  %-22s %5s | after-wait us: %6s %6s %6s | end us: %6s %6s | wait ended med" % ("class", "tiles", "median", "p90", "max", "median", "max"))
    for c in sorted(set(labels)):
        s = labels == c
        out.append("  %-22s %5d |                %6.2f %6.2f %6.2f |         %6.2f %6.2f | %6.2f"
                   % (c, s.sum(), np.median(after[s]), np.percentile(after[s], 90), after[s].max(), np.median(end[s]), end[s].max(),
                      np.median(wait_end[s])))
    for title, s in (("all tiles", np.ones(len(tiles), bool)), ("bias tiles", (tiles[:, 11] & 0x100) != 0),
                     ("ragged-column tiles", (tiles[:, 11] & 0x200) != 0), ("plain tiles", (tiles[:, 11] & 0x300) == 0)):
        if s.any():
            out.append("  %-22s %5d |                %6.2f %6.2f %6.2f |         %6.2f %6.2f | %6.2f"
                       % (title, s.sum(), np.median(after[s]), np.percentile(after[s], 90), after[s].max(), np.median(end[s]), end[s].max(),
                          np.median(wait_end[s])))
    xcd = (tiles[:, 11] >> 12) & 15
    out.append("  per XCD, last end us: " + "  ".join("%d: %.2f (%d tiles)" % (x, end[xcd == x].max(), (xcd == x).sum()) for x in sorted(set(xcd.tolist()))))
    order = np.argsort(end)[::-1][:10]
    out.append("  last ten tiles of the launch (end us, after-wait us, XCD, class):")
    for k in order:
        out.append("    %6.2f %6.2f  xcd %d  %s" % (end[k], after[k], xcd[k], labels[k]))


if __name__ == "__main__":
    lines = ["library: " + os.path.basename(os.environ.get("DSACT_LIB_PATH", "dsac-v2_amd/lib/libdsact.so"))]
    for stage in ("chain_bwd_qt", "chain_bwd_qpt"):
        report(stage, run(stage), lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
