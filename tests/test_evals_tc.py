"""evals.py --tc 1: the argument checks on the CPU; on the MI355X `TemporalConsistency` in-process against a RAFT plan
and a restatement of the test's own, and the script end to end against the formulas of its summary and against a --tc 0 run.

Gates: the flows must be the bits of a second `RaftPlan` (same weights, same precision) run on `zt_raft_pack_pair` of the two
ground-truth frames in the stated order -- (gt_t, gt_{t-1}) for the backward flow, (gt_{t-1}, gt_t) for the forward flow -- which
pins the direction of each; the table cells follow tests/test_temporal.py (count equal, sums within relative 1e-9 of the numpy
float32 restatement evaluated on those flows: 128 * 160 = 2e4 fp64 additions in another order)."""
import importlib
import json
import math

import numpy as np
import pytest
import torch

from test_evals_y4m import H, W, THRESHOLD, _payloads, _run, _weights, _write, _y4m
from test_temporal import _close, restate


# ------------------------------------------------------------------------------------------------- argument checks (no device)
_Y4M = ("--y4m_in", "LOW", "--y4m_gt", "GT", "--graph", "1")


@pytest.mark.parametrize("extra,words", [
    (("--tc", "1"), ("--tc 1 needs --y4m_in",)),
    (("--tc_scale", "2"), ("--tc_scale needs --tc 1",)),
    (("--tc_raft_weights", "RW"), ("--tc_raft_weights needs --tc 1",)),
    (_Y4M + ("--tc", "0", "--tc_scale", "2"), ("--tc_scale needs --tc 1",)),
    (_Y4M + ("--tc_raft_weights", "RW"), ("--tc_raft_weights needs --tc 1",)),
    (_Y4M + ("--tc", "1", "--tc_scale", "0"), ("--tc_scale is an integer >= 1", "got 0")),
    (_Y4M + ("--tc", "1", "--tc_scale", "-3"), ("--tc_scale is an integer >= 1", "got -3")),
    (_Y4M + ("--tc", "1", "--of_scale", "0"), ("--tc_scale is an integer >= 1", "got 0")),
    (_Y4M + ("--tc", "1", "--tc_raft_weights", "MISSING"), ("--tc_raft_weights", "MISSING: no such file")),
    (_Y4M + ("--tc", "2"), ("--tc", "invalid choice")),
], ids=["tc-alone", "scale-alone", "weights-alone", "scale-tc0", "weights-tc0", "scale-0", "scale-negative", "scale-from-of_scale",
        "weights-missing", "tc-2"])
def test_tc_argument_checks(tmp_path, extra, words):
    """every rule is a parser error that names the flag, before anything touches the device and before --save is created"""
    for name in ("LOW", "GT", "RW"):
        (tmp_path / name).write_bytes(b"")
    extra = [str(tmp_path / a) if a in ("LOW", "GT", "RW", "MISSING") else a for a in extra]
    r = _run("evals.py", "--save", tmp_path / "out", *extra, ok=False)
    assert r.returncode == 2, (r.returncode, r.stderr[-800:])
    for w in words:
        assert w in r.stderr, (w, r.stderr[-800:])
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------------------------ in-process
def _raft_state(synth, seed):
    return {k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(seed).items() if k.startswith("raft.")}


@pytest.mark.gpu
@pytest.mark.parametrize("from_file", [False, True], ids=["checkpoint", "file"])
def test_temporal_consistency_in_process(tmp_path, synth, hip_ops, from_file):
    ops, dev = hip_ops
    temporal = importlib.import_module("zero-tig_amd.temporal")
    raft = importlib.import_module("zero-tig_amd.raft")
    state = _raft_state(synth, 5 if from_file else 3)
    mine = {k: v.to(dev) for k, v in state.items()}
    if from_file:                                           # the reference's key names behind DataParallel's prefix
        path = tmp_path / "raft.pth"
        torch.save({"module." + k[5:]: v for k, v in state.items()}, str(path))
        like = {k[5:]: v for k, v in _raft_state(synth, 3).items()}
        given = temporal.load_raft_weights(str(path), like, dev)
        assert set(given) == {k for k in mine if not k.endswith("num_batches_tracked")}
    else:
        given = {k: v.clone() for k, v in mine.items()}
    tc = temporal.TemporalConsistency(ops, given, dev, H, W, 1, "bf16")
    own = raft.RaftPlan(ops, mine, dev, precision="bf16")

    def own_flow(a, b):
        x2 = torch.empty((2, H, W, 8), dtype=torch.bfloat16, device=dev)
        ops.lib.call("zt_raft_pack_pair", (a * 255.0).contiguous(), (b * 255.0).contiguous(), x2, 1, 8, H, W, H, W, None)
        return own.run(x2, iters=12)[1]

    def frame(fn, t):
        a = np.asarray(fn(t, H, W, 2), dtype=np.float32)
        return torch.from_numpy(np.ascontiguousarray(a.reshape(1, 3, H, W))).to(dev)
    outs = [frame(synth.lowlight_frame, t) for t in range(5)]
    gts = [frame(synth.clean_frame, t) for t in range(5)]
    RESET_AT = 3
    static_out, static_gt = torch.empty_like(outs[0]), torch.empty_like(gts[0])     # overwritten every frame, as the step's buffers
    for t in range(5):
        if t in (0, RESET_AT):
            tc.reset()
        static_out.copy_(outs[t])
        static_gt.copy_(gts[t])
        ri = torch.full((4,), -1, dtype=torch.int64, device=dev)
        rf = torch.full((8,), -1.0, dtype=torch.float64, device=dev)
        pushed = tc.push(static_out, static_gt, ri[1:3], rf[1:7])
        static_out.fill_(0.5), static_gt.fill_(0.5)          # what was pushed must not live in the caller's buffers
        if t in (0, RESET_AT):
            assert pushed is False and ri.tolist() == [-1] * 4 and rf.tolist() == [-1.0] * 8
            continue
        assert pushed is True
        fb, ff = own_flow(gts[t], gts[t - 1]), own_flow(gts[t - 1], gts[t])
        assert tc.fb.shape == (1, 2, H, W) and torch.equal(tc.fb, fb) and torch.equal(tc.ff, ff), t
        assert not torch.equal(fb, ff)
        nfb, nff = fb[0].cpu().numpy(), ff[0].cpu().numpy()
        gi, gf = ri.tolist(), rf.tolist()
        assert gi[0] == -1 and gi[3] == -1 and gf[0] == -1.0 and gf[7] == -1.0
        for k, seq in enumerate((outs, gts)):
            n_ref, s_ref = restate(seq[t][0].cpu().numpy(), seq[t - 1][0].cpu().numpy(), nfb, nff, 0, 0)[:2]
            got = gf[1 + 3 * k:4 + 3 * k]
            print("frame %d %s: n %d ref %d, sums %r ref %r" % (t, ("output", "gt")[k], gi[1 + k], n_ref, got, s_ref))
            assert gi[1 + k] == n_ref
            assert all(_close(a, b) for a, b in zip(got, s_ref)), (got, s_ref)
            assert all(math.isfinite(v) for v in got) and got[1] > 0 and got[2] > 0
    assert tc.pairs == 3


# ------------------------------------------------------------------------------------------------------------ end to end
def _clip(tmp_path, synth, frames):
    head = _y4m().Header(W, H, "25:1", "p", None, "420mpeg2", "LIMITED")
    fmt = head.format("bt709")
    src = _write(tmp_path / "low.y4m", head, _payloads(synth, fmt, frames, False))
    ref = _write(tmp_path / "gt.y4m", head, _payloads(synth, fmt, frames, True))
    return ("--model_pretrain", _weights(tmp_path, synth), "--graph", "1", "--precision", "bf16", "--of_scale", "1", "--y4m_in", src,
            "--y4m_gt", ref)


@pytest.mark.gpu
def test_evals_tc_end_to_end(tmp_path, synth):
    FRAMES, CUT = 6, 3
    common = _clip(tmp_path, synth, [(t, 2 if t < CUT else 7) for t in range(FRAMES)]) + ("--y4m_scene_cut", THRESHOLD)
    out = {}
    for tc in (1, 0):
        fj = tmp_path / ("frames%d.json" % tc)
        r = _run("evals.py", *common, "--save", tmp_path / ("ev%d" % tc), "--y4m_frames_json", fj, "--tc", tc)
        out[tc] = (json.load(open(str(tmp_path / ("ev%d" % tc) / "Metrics.json"))), json.load(open(str(fj))), r.stdout)
    (m, rec, _), (m0, rec0, _) = out[1], out[0]
    print(m["temporal"])
    # grading does not disturb the model: everything else is what --tc 0 reports, which has no temporal key at all
    assert "temporal" not in m0 and all("TC" not in f for f in rec0)
    assert {k: v for k, v in m.items() if k != "temporal"} == m0
    assert [{k: v for k, v in f.items() if k != "TC"} for f in rec] == rec0
    assert m["cuts"] == [CUT] and m["images"] == FRAMES
    # the pairs: every frame but the first and the cut frame
    te, px = m["temporal"], H * W
    assert [f["TC"] is None for f in rec] == [t in (0, CUT) for t in range(FRAMES)]
    pairs = [f["TC"] for f in rec if f["TC"] is not None]
    assert te["pairs"] == FRAMES - 1 - len(m["cuts"]) == len(pairs)
    assert te["scale"] == 1 and te["size"] == [W, H] and te["raft"] == "checkpoint"
    n = sum(p["N"] for p in pairs)
    assert all(isinstance(p["N"], int) and 0 <= p["N"] <= px and len(p["out"]) == 3 and len(p["gt"]) == 3 for p in pairs)
    assert all(math.isfinite(v) for p in pairs for v in p["out"] + p["gt"])
    assert te["valid_share"] == n / (len(pairs) * px) and 0 < te["valid_share"] <= 1
    for sfx, key in (("", "out"), ("_gt", "gt")):
        s = [sum(p[key][q] for p in pairs) for q in range(3)]
        assert te["E_warp" + sfx] == s[0] / (3 * n)
        assert te["E_static" + sfx] == s[1] / (3 * len(pairs) * px)
        assert te["MABD" + sfx] == s[2] / (3 * len(pairs) * px)
    assert te["MABD_mse"] == sum((p["out"][2] / (3 * px) - p["gt"][2] / (3 * px)) ** 2 for p in pairs) / len(pairs)
    assert te["E_static_gt"] > 0 and all(math.isfinite(te[k]) for k in te if k.startswith(("E_", "MABD")))
    assert set(te) == {"scale", "size", "pairs", "raft", "valid_share", "E_warp", "E_static", "MABD", "E_warp_gt", "E_static_gt",
                       "MABD_gt", "MABD_mse"}


@pytest.mark.gpu
def test_evals_tc_too_small_for_raft(tmp_path, synth):
    """128 x 160 at --tc_scale 3 is 42 x 53: temporal is switched off, one log line says why, everything else is graded"""
    common = _clip(tmp_path, synth, [(t, 2) for t in range(3)])
    fj = tmp_path / "frames.json"
    r = _run("evals.py", *common, "--save", tmp_path / "ev", "--hist_match", "0", "--y4m_frames_json", fj, "--tc", "1", "--tc_scale", "3")
    m, rec = json.load(open(str(tmp_path / "ev" / "Metrics.json"))), json.load(open(str(fj)))
    assert "temporal" in m and m["temporal"] is None and m["images"] == 3 and math.isfinite(m["Total_PSNR"])
    assert all("TC" in f and f["TC"] is None for f in rec)
    assert sum("temporal metrics off" in line for line in r.stdout.split("\n")) == 1, r.stdout[-2000:]
