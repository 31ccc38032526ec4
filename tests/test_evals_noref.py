"""evals.py --noref 1: the argument checks and the host-side formulas on the CPU; on the MI355X the script end to end
against the formulas of its summary, `Ops.noref` on an InferStep's own tensors against the numpy restatement of
tests/test_noref.py (integers equal), and --tc 1 with the flows taken from the output."""
import importlib
import json
import math

import numpy as np
import pytest
import torch

from test_evals_y4m import H, W, THRESHOLD, _payloads, _run, _weights, _write, _y4m
from test_metrics import SSIM_TOL
from test_noref import from_hist, joint_hist, lightness

KEYS = ("LOE", "LOE_50", "L_in", "L_out", "gain", "entropy_in", "entropy_out", "sat_out", "black_out")


# ------------------------------------------------------------------------------------------------- argument checks (no device)
@pytest.mark.parametrize("extra,words", [
    (("--noref", "1"), ("--noref 1 needs --y4m_in",)),
    (("--noref", "1", "--graph", "1"), ("--noref 1 needs --y4m_in",)),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "1", "--y4m_gt", "GT"), ("--noref 1", "--y4m_gt cannot be combined")),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "1", "--lpips_weights", "LW"), ("--noref 1", "--lpips_weights cannot be combined")),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "1", "--hist_match", "1"), ("--noref 1", "--hist_match 1 cannot be combined")),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "0"), ("--y4m_in needs --y4m_gt",)),
    (("--y4m_in", "LOW", "--graph", "1"), ("--y4m_in needs --y4m_gt",)),
    (("--y4m_in", "LOW", "--graph", "0", "--noref", "1"), ("--y4m_in needs --graph 1", "--graph is 0")),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "1", "--save_images", "3"), ("--save_images cannot be combined",)),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "1", "--y4m_size", "1920"), ("--y4m_size takes WxH",)),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "1", "--y4m_cuts_json", "C"), ("--y4m_cuts_json needs --y4m_scene_cut",)),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "1", "--tc_scale", "2"), ("--tc_scale needs --tc 1",)),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "2"), ("--noref", "invalid choice")),
], ids=["noref-alone", "noref-graph", "with-gt", "with-lpips", "with-hist_match", "noref0-in-alone", "in-alone", "graph0", "save_images",
        "size-1920", "cuts_json-alone", "tc_scale-alone", "noref-2"])
def test_noref_argument_checks(tmp_path, extra, words):
    """every rule is a parser error that names its flags, before anything touches the device and before --save is created"""
    for name in ("LOW", "GT", "LW"):
        (tmp_path / name).write_bytes(b"")
    extra = [str(tmp_path / a) if a in ("LOW", "GT", "LW", "C") else a for a in extra]
    r = _run("evals.py", "--save", tmp_path / "out", *extra, ok=False)
    assert r.returncode == 2, (r.returncode, r.stderr[-800:])
    for w in words:
        assert w in r.stderr, (w, r.stderr[-800:])
    assert not (tmp_path / "out").exists()


def test_noref_host_formulas():
    evals = importlib.import_module("evals")
    assert evals.loe50_grid(1080, 1920) == (50, 89) and evals.loe50_grid(1920, 1080) == (89, 50)     # 88.89 -> 89
    assert evals.loe50_grid(128, 160) == (50, 63) and evals.loe50_grid(100, 101) == (50, 51)         # 62.5 -> 63 (half up), 50.5 -> 51
    assert evals.loe50_grid(7, 7) == (50, 50) and evals.loe50_grid(1, 1) == (50, 50)
    v = evals.noref_values([1, 0, 3, 9, 0, 0], [0.0, 0.0], [2500, 0, 7500, 22500, 0, 0])
    assert v["LOE"] is None and v["LOE_50"] == 0.0 and v["L_in"] == 3.0 and v["L_out"] == 9.0 and v["gain"] == 3.0
    v = evals.noref_values([10, 18, 0, 50, 1, 2], [0.0, 1.5], [4, 6, 0, 20, 0, 0])
    assert v == {"LOE": 18 / 90, "LOE_50": 1.5, "L_in": 0.0, "L_out": 5.0, "gain": None, "entropy_in": 0.0, "entropy_out": 1.5,
                 "sat_out": 0.1, "black_out": 0.2}
    assert tuple(v) == KEYS == evals.NR_KEYS


# ----------------------------------------------------------------------------------------------------------- end to end
def _low_clip(tmp_path, synth, frames):
    head = _y4m().Header(W, H, "25:1", "p", None, "420mpeg2", "LIMITED")
    fmt = head.format("bt709")
    src = _write(tmp_path / "low.y4m", head, _payloads(synth, fmt, frames, False))
    return ("--model_pretrain", _weights(tmp_path, synth), "--graph", "1", "--precision", "bf16", "--of_scale", "1", "--y4m_in", src,
            "--noref", "1"), fmt


@pytest.mark.gpu
def test_evals_noref_end_to_end(tmp_path, synth):
    FRAMES, CUT = 9, 5
    common, _ = _low_clip(tmp_path, synth, [(t, 2 if t < CUT else 7) for t in range(FRAMES)])
    fj = tmp_path / "frames.json"
    r = _run("evals.py", *common, "--save", tmp_path / "ev", "--y4m_frames_json", fj, "--y4m_scene_cut", THRESHOLD)
    m, rec = json.load(open(str(tmp_path / "ev" / "Metrics.json"))), json.load(open(str(fj)))
    print(m)
    for k in ("Total_PSNR", "Total_SSIM", "Total_LPIPS", "Total_PSNR_HM", "Total_SSIM_HM", "Total_LPIPS_HM", "planes"):
        assert k in m and m[k] is None, (k, m)
    assert m["images"] == FRAMES and m["cuts"] == [CUT] and "temporal" not in m
    assert len(rec) == FRAMES and [f["frame"] for f in rec] == list(range(FRAMES)) and [f["cut"] for f in rec] == [t == CUT for t in range(FRAMES)]
    nr = m["noref"]
    assert set(nr) == set(KEYS) | {"graded"} and nr["graded"] == "denoise"
    evals = importlib.import_module("evals")
    gh, gw = evals.loe50_grid(H, W)
    for f in rec:
        v, full, sub = f["noref"], f["noref"]["ints"], f["noref"]["ints_50"]
        assert set(v) == set(KEYS) | {"ints", "ints_50"} and "PSNR" not in f
        assert full[0] == H * W and sub[0] == gh * gw and all(isinstance(x, int) and x >= 0 for x in full + sub)
        assert {k: v[k] for k in KEYS} == evals.noref_values(full, [v["entropy_in"], v["entropy_out"]], sub)
        assert 0.0 <= v["LOE"] <= 1.0 and 0.0 <= v["LOE_50"] <= gh * gw
        assert 0.0 <= v["L_in"] <= 255.0 and 0.0 <= v["L_out"] <= 255.0 and v["gain"] == v["L_out"] / v["L_in"]
        assert 0.0 <= v["entropy_in"] <= 8.0 and 0.0 <= v["entropy_out"] <= 8.0
        assert 0.0 <= v["sat_out"] <= 1.0 and 0.0 <= v["black_out"] <= 1.0
    # the totals: the mean over the frames of each per-frame value, summed in frame order; the gain is that of the stream
    for k in KEYS:
        if k != "gain":
            assert nr[k] == sum(f["noref"][k] for f in rec) / FRAMES, (k, nr[k])
    assert nr["gain"] == sum(f["noref"]["ints"][3] for f in rec) / sum(f["noref"]["ints"][2] for f in rec)
    assert sum(line.split(" ", 3)[-1].startswith("NUM: %d, LOE: " % FRAMES) for line in r.stdout.split("\n")) == 1, r.stdout[-2000:]
    assert "Total LOE: " in r.stdout and "PSNR" not in r.stdout


@pytest.mark.gpu
def test_noref_on_infer_step_tensors(tmp_path, synth, hip_ops):
    """Ops.noref(step.x, output) on two frames of an InferStep against the restatement applied to the same tensors copied to the host"""
    ops, dev = hip_ops
    evals = importlib.import_module("evals")
    common, fmt = _low_clip(tmp_path, synth, [(t, 2) for t in range(2)])
    args = evals.parser.parse_args([str(a) for a in common])
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    model = evals.Finetunemodel(args).to(dev)
    model.eval()
    for p in model.parameters():
        p.requires_grad = False
    step = importlib.import_module("zero-tig_amd.infer").InferStep(model, use_graph=True, ingest_size=None, yuv=fmt, yuv_out_depth=fmt.depth)
    low = _payloads(synth, fmt, [(t, 2) for t in range(2)], False)
    with torch.no_grad():
        for t, p in enumerate(low):
            _, output, _ = step(torch.from_numpy(p.copy()).pin_memory(), t == 0)
            assert tuple(step.x.shape) == (1, 3, H, W) and step.x.shape == output.shape
            for grid in (None, evals.loe50_grid(H, W)):
                oi, of = ops.noref(step.x, output, grid)
                a, b = step.x[0].cpu().numpy(), output[0].cpu().numpy()
                ints, ents = from_hist(joint_hist(*lightness(a, b, grid)))
                print("frame %d grid %r: %r ref %r, %r ref %r" % (t, grid, oi.tolist(), ints, of.tolist(), ents))
                assert oi.tolist() == ints and ints[0] == (H * W if grid is None else grid[0] * grid[1])
                for g, w in zip(of.tolist(), ents):
                    assert abs(g - w) <= SSIM_TOL * max(abs(w), 1.0), (g, w)


@pytest.mark.gpu
def test_evals_noref_tc(tmp_path, synth):
    FRAMES = 4
    common, _ = _low_clip(tmp_path, synth, [(t, 2) for t in range(FRAMES)])
    fj = tmp_path / "frames.json"
    _run("evals.py", *common, "--save", tmp_path / "ev", "--y4m_frames_json", fj, "--tc", "1")
    m, rec = json.load(open(str(tmp_path / "ev" / "Metrics.json"))), json.load(open(str(fj)))
    te = m["temporal"]
    print(te)
    assert te["flow_from"] == "output" and te["pairs"] == FRAMES - 1 and te["scale"] == 1 and te["size"] == [W, H]
    for k in ("E_warp_gt", "E_static_gt", "MABD_gt", "MABD_mse"):
        assert k in te and te[k] is None, (k, te)
    assert all(math.isfinite(te[k]) and te[k] >= 0 for k in ("E_warp", "E_static", "MABD")) and 0 < te["valid_share"] <= 1
    assert [f["TC"] is None for f in rec] == [t == 0 for t in range(FRAMES)]
    pairs = [f["TC"] for f in rec if f["TC"] is not None]
    assert all(p["gt"] is None and len(p["out"]) == 3 for p in pairs)
    n = sum(p["N"] for p in pairs)
    assert te["E_warp"] == sum(p["out"][0] for p in pairs) / (3 * n)
    assert m["noref"]["graded"] == "denoise" and m["images"] == FRAMES and m["Total_PSNR"] is None
