"""evals.py --color 1: the argument checks, the host formulas and the grader's bookkeeping on the CPU; on the MI355X the
script end to end (--noref 1 and --y4m_gt, and the PNG loop) against the formulas of its summary, `Ops.color_stats` on an
InferStep's own tensors against the numpy restatement of tests/test_color.py, and `utils.color_quality` against the grader."""
import importlib
import json
import logging
import math
import types

import numpy as np
import pytest
import torch

from test_color import restate
from test_evals_noref import _low_clip
from test_evals_tc import _clip
from test_evals_y4m import H, W, _payloads, _run, _weights
from test_grading import _messages, _result, _row
from test_metrics import SSIM_TOL

grading = importlib.import_module("zero-tig_amd.grading")
KEYS = ("UIQM", "UICM", "UISM", "UIConM", "UCIQE", "sigma_c", "con_l", "mu_s", "colorfulness", "mean_rgb")
ONE_PIXEL = ([1, 0, 10, 20, 30, -10, 100, 0, -30, 900, 0, 0, 500, 500, 0, 0, 0, 0], [5.0, 25.0, 0.5, 0.0, 0.0, 0.0, 0.0])
ONE_BLOCK = ([100, 1, 300, 100, 150, 200, 800, 160, 0, 1600, 0, 80, 100, 600, 0, 0, 1, 0], [1000.0, 12500.0, 25.0, 2.0, 1.0, 0.0, -0.5])


# ------------------------------------------------------------------------------------------------- argument checks (no device)
@pytest.mark.parametrize("extra,words", [
    (("--color_block", "8"), ("--color_block needs --color 1",)),
    (("--color", "0", "--color_block", "8"), ("--color_block needs --color 1",)),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "1", "--color_block", "8"), ("--color_block needs --color 1",)),
    (("--color", "1", "--color_block", "3"), ("--color_block", "4..64", "got 3")),
    (("--y4m_in", "LOW", "--graph", "1", "--noref", "1", "--color", "1", "--color_block", "65"), ("--color_block", "4..64", "got 65")),
    (("--color", "2"), ("--color", "invalid choice")),
    (("--y4m_in", "LOW", "--graph", "1", "--color", "1"), ("--y4m_in needs --y4m_gt",)),
], ids=["block-alone", "block-color0", "block-noref", "block-3", "block-65", "color-2", "color-needs-gt-or-noref"])
def test_color_argument_checks(tmp_path, extra, words):
    (tmp_path / "LOW").write_bytes(b"")
    extra = [str(tmp_path / a) if a == "LOW" else a for a in extra]
    r = _run("evals.py", "--save", tmp_path / "out", *extra, ok=False)
    assert r.returncode == 2, (r.returncode, r.stderr[-800:])
    for w in words:
        assert w in r.stderr, (w, r.stderr[-800:])
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------------------- host formulas (no device)
def test_color_host_formulas():
    evals = importlib.import_module("evals")
    assert evals.color_values is grading.color_values and evals.COLOR_KEYS is grading.COLOR_KEYS and tuple(grading.COLOR_KEYS) == KEYS
    v = grading.color_values(*ONE_PIXEL, 10)                 # n_kept = 0 and nblk = 0: the four measures that need them are null
    assert tuple(v) == KEYS
    assert v["UIQM"] is None and v["UICM"] is None and v["UISM"] is None and v["UIConM"] is None
    assert v["sigma_c"] == 0.0 and v["con_l"] == 0.0 and v["mu_s"] == 0.5 and v["UCIQE"] == 0.2576 * 0.5
    assert v["colorfulness"] == 0.3 * math.hypot(10.0, 15.0) and v["mean_rgb"] == [10.0, 20.0, 30.0]
    v = grading.color_values(*ONE_BLOCK, 10)
    # mu_rg = 160 / 80 = 2, var_rg = 8 - 2 * 2 * 2 + 4 = 4; mu_yb = 0, var_yb = 1600 / 400 = 4
    uicm, uism, uiconm = -0.0268 * 2.0 + 0.1586 * math.sqrt(8.0), 0.299 * 2.0 + 0.587 * 1.0, 0.5
    assert v["UICM"] == pytest.approx(uicm, rel=1e-14) and v["UISM"] == pytest.approx(uism, rel=1e-14) and v["UIConM"] == uiconm
    assert v["UIQM"] == pytest.approx(0.0282 * uicm + 0.2953 * uism + 3.5753 * uiconm, rel=1e-14)
    assert v["sigma_c"] == pytest.approx(5.0 / 255.0, rel=1e-14) and v["con_l"] == 0.5 and v["mu_s"] == 0.25
    assert v["UCIQE"] == pytest.approx(0.4680 * 5.0 / 255.0 + 0.2745 * 0.5 + 0.2576 * 0.25, rel=1e-14)
    assert v["colorfulness"] == pytest.approx(math.sqrt(8.0) + 0.3 * 2.0, rel=1e-14) and v["mean_rgb"] == [3.0, 1.0, 1.5]
    # the trimmed mean is not the mean: the spread is taken about it
    ints = list(ONE_BLOCK[0])
    ints[7] = 0                                             # T_rg = 0: mu_rg = 0, var_rg = S2 / N = 8
    assert grading.color_values(ints, ONE_BLOCK[1], 10)["UICM"] == pytest.approx(0.1586 * math.sqrt(12.0), rel=1e-14)
    with pytest.raises(AssertionError):                     # two blocks of 10 x 10 do not fit into 100 pixels
        grading.color_values([100, 2] + ints[2:], ONE_BLOCK[1], 10)


def test_color_grader(caplog):
    """frame 1 is the one-pixel row (no UIQM), frame 2 the one-block row: each mean is over the frames that have a value"""
    caplog.set_level(logging.INFO)
    tab = grading.MetricTable(None, 64)
    g = grading.ColorGrader(tab, None, 10, ("out", "in"))
    assert tab.width == {torch.int64: 36, torch.float64: 14}
    rows = []
    for a, b in ((ONE_PIXEL, ONE_BLOCK), (ONE_BLOCK, ONE_BLOCK)):
        rows.append(_row(tab, [("i", g.cols["out"][0], a[0]), ("f", g.cols["out"][1], a[1]), ("i", g.cols["in"][0], b[0]),
                               ("f", g.cols["in"][1], b[1])]))
    recs = [{"frame": 0, "cut": False}, {"frame": 1, "cut": False}]
    for n, (rec, (ri, rf)) in enumerate(zip(recs, rows), 1):
        g.read(n, rec, ri, rf)
    one, blk = grading.color_values(*ONE_PIXEL, 10), grading.color_values(*ONE_BLOCK, 10)
    assert recs[0]["color"] == {"out": dict(one, ints=ONE_PIXEL[0], sums=ONE_PIXEL[1]), "in": dict(blk, ints=ONE_BLOCK[0], sums=ONE_BLOCK[1])}
    assert list(recs[0]["color"]["out"]) == list(KEYS) + ["ints", "sums"] and list(recs[1]["color"]) == ["out", "in"]
    lines = _messages(caplog)
    assert len(lines) == 4 and lines[0].startswith("NUM: 1, color out: UIQM: null, UICM: null, UISM: null, UIConM: null, UCIQE: 0.1288")
    assert lines[3].startswith("NUM: 2, color in: UIQM: %.4f, " % blk["UIQM"])
    caplog.clear()
    result = _result(2, color=None)
    g.blocks = [1, 1]
    g.summary(result)
    co = result["color"]
    assert list(co) == ["block", "graded", "blocks", "out", "in", "gt"] and list(result) == list(_result(2, color=None))
    assert co["block"] == 10 and co["graded"] == "denoise" and co["blocks"] == [1, 1] and co["gt"] is None and co["in"] == blk
    for k in KEYS:
        if one[k] is None:
            assert co["out"][k] == blk[k], k                # one frame has a value: the mean is that value
        elif k == "mean_rgb":
            assert co["out"][k] == [(x + y) / 2 for x, y in zip(one[k], blk[k])]
        else:
            assert co["out"][k] == (one[k] + blk[k]) / 2, k
    assert len(_messages(caplog)) == 1 and _messages(caplog)[0].startswith("colour (2 frames, blocks of 10): out UIQM: ")


# ----------------------------------------------------------------------------------------------------------- end to end
def _check_block(co, rec, which, frames, block):
    """the summary is the mean over the frames that have a value; every record follows from its raw numbers"""
    assert set(co) == {"block", "graded", "blocks", "out", "in", "gt"} and co["block"] == block and co["graded"] == "denoise"
    assert co["blocks"] == [H // block, W // block]
    for f in rec:
        assert list(f["color"]) == list(which)
        for w in which:
            v = f["color"][w]
            assert set(v) == set(KEYS) | {"ints", "sums"} and len(v["ints"]) == 18 and len(v["sums"]) == 7
            assert v["ints"][0] == H * W and v["ints"][1] == (H // block) * (W // block) and all(isinstance(x, int) for x in v["ints"])
            assert {k: v[k] for k in KEYS} == grading.color_values(v["ints"], v["sums"], block)
            assert all(v[k] is not None and math.isfinite(v[k]) for k in KEYS[:-1])
            assert 0.0 <= v["con_l"] <= 1.0 and 0.0 <= v["mu_s"] <= 1.0 and v["UISM"] >= 0.0 and v["UIConM"] >= 0.0
    for w in ("out", "in", "gt"):
        if w not in which:
            assert co[w] is None
            continue
        for k in KEYS[:-1]:
            assert co[w][k] == sum(f["color"][w][k] for f in rec) / frames, (w, k)
        assert co[w]["mean_rgb"] == [sum(f["color"][w]["mean_rgb"][c] for f in rec) / frames for c in range(3)]


@pytest.mark.gpu
def test_evals_color_noref_end_to_end(tmp_path, synth):
    """--noref 1 --color 1 --color_block 8 grades "out" and "in"; without --color 1 the same command writes the same Metrics.json
    less the "color" key, and the records have no "color" """
    FRAMES = 3
    common, _ = _low_clip(tmp_path, synth, [(t, 2) for t in range(FRAMES)])
    fj, fj0 = tmp_path / "frames.json", tmp_path / "frames0.json"
    r = _run("evals.py", *common, "--save", tmp_path / "ev", "--y4m_frames_json", fj, "--color", "1", "--color_block", "8")
    _run("evals.py", *common, "--save", tmp_path / "ev0", "--y4m_frames_json", fj0)
    m, rec = json.load(open(str(tmp_path / "ev" / "Metrics.json"))), json.load(open(str(fj)))
    m0, rec0 = json.load(open(str(tmp_path / "ev0" / "Metrics.json"))), json.load(open(str(fj0)))
    print(m["color"])
    assert "color" not in m0 and all("color" not in f for f in rec0)
    assert {k: v for k, v in m.items() if k != "color"} == m0 and list(m)[-1] == "color"
    assert [{k: v for k, v in f.items() if k != "color"} for f in rec] == rec0
    _check_block(m["color"], rec, ("out", "in"), FRAMES, 8)
    lines = [line.split(" ", 3)[-1] for line in r.stdout.split("\n")]
    assert sum(line.startswith("NUM: %d, color out: UIQM: " % FRAMES) for line in lines) == 1, r.stdout[-2000:]
    assert sum(line.startswith("NUM: %d, color in: UIQM: " % FRAMES) for line in lines) == 1
    assert sum(line.startswith("colour (%d frames, blocks of 8): out UIQM: " % FRAMES) for line in lines) == 1


@pytest.mark.gpu
def test_evals_color_with_ground_truth(tmp_path, synth):
    """--y4m_gt --color 1: the ground truth is graded as well, with the default block of 10; the clean twin is more colourful than
    the dark input"""
    FRAMES = 2
    common = _clip(tmp_path, synth, [(t, 2) for t in range(FRAMES)])
    fj = tmp_path / "frames.json"
    _run("evals.py", *common, "--save", tmp_path / "ev", "--y4m_frames_json", fj, "--color", "1", "--hist_match", "0")
    m, rec = json.load(open(str(tmp_path / "ev" / "Metrics.json"))), json.load(open(str(fj)))
    print(m["color"])
    _check_block(m["color"], rec, ("out", "in", "gt"), FRAMES, 10)
    assert m["color"]["gt"]["colorfulness"] > m["color"]["in"]["colorfulness"]
    assert m["Total_PSNR"] is not None and "PSNR" in rec[0]


@pytest.mark.gpu
def test_color_on_infer_step_tensors(tmp_path, synth, hip_ops):
    """Ops.color_stats on an InferStep's input and output against the restatement applied to the same tensors copied to the host,
    and utils.color_quality against the grader's numbers for the same frame"""
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
    tab = grading.MetricTable(dev, 2)
    grader = grading.ColorGrader(tab, ops, 10, ("out", "in"))
    tab.build()
    with torch.no_grad():
        for t, p in enumerate(low):
            _, output, _ = step(torch.from_numpy(p.copy()).pin_memory(), t == 0)
            ri, rf = tab.row(t)
            grader.launch(types.SimpleNamespace(step=step, output=output, gt=None), ri, rf)
            for name, frame in (("out", output), ("in", step.x)):
                ints, floats = restate(frame[0].cpu().numpy(), 10)
                ci, cf = grader.cols[name]
                gi, gf = ri[ci].tolist(), rf[cf].tolist()
                print("frame %d %s: %r ref %r, %r ref %r" % (t, name, gi, ints, gf, floats))
                assert gi == ints and ints[0] == H * W
                for g, w in zip(gf, floats):
                    assert abs(g - w) <= SSIM_TOL * max(abs(w), 1.0), (g, w)
                assert evals.utils.color_quality(frame, 10) == grading.color_values(gi, gf, 10)
    assert grader.blocks == [H // 10, W // 10]


@pytest.mark.gpu
def test_evals_color_dataset_mode(tmp_path, synth):
    """the PNG loop with two pairs: "out" and "gt" are the means of `utils.color_quality` over the pairs, "in" is null; the ground
    truth's numbers are recomputed here from the files"""
    from PIL import Image
    evals = importlib.import_module("evals")
    data = tmp_path / "data" / "RLV"
    paths = []
    for kind, sub, fn in (("input", "low_light_10", synth.lowlight_frame), ("gt", "normal_light_10", synth.clean_frame)):
        d = data / kind / "S01" / sub
        d.mkdir(parents=True)
        for t in range(2):
            a = np.asarray(fn(t, 135, 240), dtype=np.float32)
            im = (np.transpose(a[0] if a.ndim == 4 else a, (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8)
            Image.fromarray(im).save(str(d / ("%05d.png" % (t + 1))))
            if kind == "gt":
                paths.append(str(d / ("%05d.png" % (t + 1))))
    (data / "train_list.txt").write_text("S01\n")
    (data / "test_list.txt").write_text("S01\n")
    common = ("--dataset", "RLV", "--lowlight_images_path", data, "--model_pretrain", _weights(tmp_path, synth), "--hist_match", "0",
              "--save_images", "0")
    r = _run("evals.py", *common, "--save", tmp_path / "ev", "--color", "1")
    _run("evals.py", *common, "--save", tmp_path / "ev0")
    m, m0 = json.load(open(str(tmp_path / "ev" / "Metrics.json"))), json.load(open(str(tmp_path / "ev0" / "Metrics.json")))
    print(m["color"])
    assert "color" not in m0 and {k: v for k, v in m.items() if k != "color"} == m0
    co = m["color"]
    assert list(co) == ["block", "graded", "blocks", "out", "in", "gt"] and co["block"] == 10 and co["blocks"] == [108, 192]
    assert co["in"] is None and set(co["out"]) == set(KEYS) == set(co["gt"])
    dev = torch.device("cuda", 0)
    want = [evals.utils.color_quality(evals.utils.ingest_frame(torch.from_numpy(np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8).copy()),
                                                               dev), 10) for p in paths]
    for k in KEYS[:-1]:
        assert co["gt"][k] == (want[0][k] + want[1][k]) / 2, k
        assert math.isfinite(co["out"][k])
    assert co["gt"]["mean_rgb"] == [(want[0]["mean_rgb"][c] + want[1]["mean_rgb"][c]) / 2 for c in range(3)]
    assert "NUM: 2, color gt: UIQM: " in r.stdout and "colour (2 images, blocks of 10): out UIQM: " in r.stdout
