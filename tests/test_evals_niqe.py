"""evals.py --niqe MODEL: on the CPU the model file (round trip, key and shape errors, the .mat path with and without
scipy), `niqe_value` against `numpy.linalg.pinv` by hand, the parser error, the sharpness selection of `NiqeModel.fit` on hand-made
sums and the grader's bookkeeping; on the MI355X `tools/niqe_fit.py` on a clean clip, then the script end to end with and without
the option, "in" against `utils.niqe` of the same decoded frame, and the ordering clean < clean plus noise."""
import importlib
import json
import logging
import math
import sys
import types

import numpy as np
import pytest
import torch

from test_evals_y4m import _payloads, _run, _weights, _write, _y4m
from test_grading import _messages, _result, _row
from test_niqe import fits

grading = importlib.import_module("zero-tig_amd.grading")
NH, NW, FRAMES = 192, 288, 4                                # six blocks: the smallest frame here with more rows than the two NIQE needs


def _model(seed=0):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((36, 36))
    return grading.NiqeModel(rng.standard_normal(36), a @ a.T / 36.0, "m")


def _frame_numbers(feat):
    """features [n,36], all finite -> the 38 integers and 738 floats of the frame kernel"""
    n = feat.shape[0]
    mean = feat.mean(axis=0)
    c = feat - mean
    return [n, n] + [n] * 36, feat.sum(axis=0).tolist() + mean.tolist() + (c.T @ c)[np.triu_indices(36)].tolist()


# ------------------------------------------------------------------------------------------------------------- the model file
def test_model_round_trip_and_errors(tmp_path, monkeypatch):
    m = _model()
    path = tmp_path / "model.npz"
    m.save(str(path))
    data = np.load(str(path))
    assert sorted(data.files) == ["cov_pris_param", "mu_pris_param"] and data["mu_pris_param"].shape == (1, 36)
    back = grading.NiqeModel.load(str(path))
    assert back.name == "model.npz" and back.mu.shape == (36,) and np.array_equal(back.mu, m.mu) and np.array_equal(back.cov, m.cov)
    np.savez(str(tmp_path / "flat.npz"), mu_pris_param=m.mu, cov_pris_param=m.cov)          # [36] is accepted as well
    assert np.array_equal(grading.NiqeModel.load(str(tmp_path / "flat.npz")).mu, m.mu)
    np.savez(str(tmp_path / "keys.npz"), mu=m.mu, cov_pris_param=m.cov)
    with pytest.raises(ValueError, match=r"mu_pris_param.*\['cov_pris_param', 'mu'\]"):
        grading.NiqeModel.load(str(tmp_path / "keys.npz"))
    np.savez(str(tmp_path / "shape.npz"), mu_pris_param=m.mu[:35], cov_pris_param=m.cov)
    with pytest.raises(ValueError, match=r"\[35\].*\[36, 36\].*\['cov_pris_param', 'mu_pris_param'\]"):
        grading.NiqeModel.load(str(tmp_path / "shape.npz"))
    np.savez(str(tmp_path / "cov.npz"), mu_pris_param=m.mu, cov_pris_param=m.cov[:, :35])
    with pytest.raises(ValueError, match=r"\[36, 35\]"):
        grading.NiqeModel.load(str(tmp_path / "cov.npz"))
    from scipy.io import savemat
    savemat(str(tmp_path / "modelparameters.mat"), {"mu_prisparam": m.mu.reshape(1, 36), "cov_prisparam": m.cov})
    mat = grading.NiqeModel.load(str(tmp_path / "modelparameters.mat"))
    assert np.array_equal(mat.mu, m.mu) and np.array_equal(mat.cov, m.cov) and mat.name == "modelparameters.mat"
    savemat(str(tmp_path / "other.mat"), {"mu_pris_param": m.mu, "cov_prisparam": m.cov})
    with pytest.raises(ValueError, match=r"mu_prisparam.*\['cov_prisparam', 'mu_pris_param'\]"):
        grading.NiqeModel.load(str(tmp_path / "other.mat"))
    monkeypatch.setitem(sys.modules, "scipy.io", None)      # scipy cannot be imported
    with pytest.raises(ValueError, match="needs scipy"):
        grading.NiqeModel.load(str(tmp_path / "modelparameters.mat"))
    assert np.array_equal(grading.NiqeModel.load(str(path)).mu, m.mu)                       # the .npz path does not need it


def test_niqe_value_by_hand():
    m = _model(1)
    feat = np.random.default_rng(2).standard_normal((5, 36)) * 0.1 + 1.0
    ints, floats = _frame_numbers(feat)
    d = m.mu - feat.mean(axis=0)
    want = math.sqrt(d @ np.linalg.pinv((m.cov + np.cov(feat, rowvar=False, ddof=1)) / 2.0) @ d)
    assert grading.niqe_value(ints, floats, m) == pytest.approx(want, rel=1e-12)
    # a column with one NaN: its mean is over the other four, the row is not valid
    nan_feat = feat.copy()
    nan_feat[4, 7] = np.nan
    vi, vf = _frame_numbers(feat[:4])
    count = [5] * 36
    count[7] = 4
    ints2 = [5, 4] + count
    floats2 = np.nansum(nan_feat, axis=0).tolist() + vf[36:]
    mu_d = np.nanmean(nan_feat, axis=0)
    d = m.mu - mu_d
    want = math.sqrt(d @ np.linalg.pinv((m.cov + np.cov(feat[:4], rowvar=False, ddof=1)) / 2.0) @ d)
    assert grading.niqe_value(ints2, floats2, m) == pytest.approx(want, rel=1e-12)
    # fewer than two valid rows, a column without a value, an untouched table row: no value
    assert grading.niqe_value([5, 1] + [5] * 36, floats, m) is None
    assert grading.niqe_value([5, 4] + [0] + [5] * 35, floats, m) is None
    assert grading.niqe_value([0] * 38, [0.0] * 738, m) is None


def test_niqe_parser_error(tmp_path):
    (tmp_path / "LOW").write_bytes(b"")
    for extra in (("--niqe", tmp_path / "MISSING.npz"), ("--y4m_in", tmp_path / "LOW", "--graph", "1", "--noref", "1", "--niqe", tmp_path / "MISSING.npz")):
        r = _run("evals.py", "--save", tmp_path / "out", *extra, ok=False)
        assert r.returncode == 2 and "--niqe" in r.stderr and "MISSING.npz: no such file" in r.stderr, r.stderr[-800:]
        assert not (tmp_path / "out").exists()


def _hand_sums(sharp, sigmas):
    """blocks whose fields are roughly Gaussian with the given scale: every fit has a value"""
    n = len(sharp)
    si, sf = np.zeros((2, n, 10), dtype=np.int64), np.zeros((2, n, 16))
    for s, px in enumerate((9216, 2304)):
        for b in range(n):
            for f in range(5):
                sl, sr = sigmas[b] * (1.0 + 0.1 * f), sigmas[b] * (1.0 + 0.05 * s)
                si[s, b, 2 * f:2 * f + 2] = px // 2 - 100, px // 2 + 100
                sf[s, b, 3 * f:3 * f + 3] = (px // 2 - 100) * sl * sl, (px // 2 + 100) * sr * sr, 0.78 * px * (sl + sr) / 2.0
    sf[0, :, 15] = np.asarray(sharp) * 9216.0
    return si, sf


def test_fit_selects_the_sharp_blocks():
    a = _hand_sums([10.0, 8.0, 7.5, 7.6, 1.0], [0.5, 0.6, 0.7, 0.8, 0.9])                   # 7.5 is not greater than 0.75 * 10
    b = _hand_sums([2.0, 1.4, 1.6], [0.3, 0.4, 0.45])
    assert grading.NiqeModel.select(a[1]).tolist() == [True, True, False, True, False]
    assert grading.NiqeModel.select(b[1]).tolist() == [True, False, True]
    m = grading.NiqeModel.fit([a, b], "hand")
    fa, fb = fits(*a)[0], fits(*b)[0]                       # the restatement's fit, full argmin
    rows = np.concatenate([fa[[0, 1, 3]], fb[[0, 2]]])
    assert np.all(np.isfinite(rows)) and m.blocks == (5, 5) and m.name == "hand"
    np.testing.assert_allclose(m.mu, rows.mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(m.cov, np.cov(rows, rowvar=False, ddof=1), rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(grading.niqe_features(*a), fa, rtol=1e-12)
    # a block without a fit: its NaN features stay out of the covariance, the other columns of the row count in mu
    c = (a[0].copy(), a[1].copy())
    c[0][1, 0, 4] = 0                                       # scale 2, block 0, field 2: n_neg = 0
    mc = grading.NiqeModel.fit([c, b], "hand")
    fc = fits(*c)[0]
    assert int(np.isnan(fc[0]).sum()) == 4 and mc.blocks == (4, 5)
    rows_c = np.concatenate([fc[[0, 1, 3]], fb[[0, 2]]])
    np.testing.assert_allclose(mc.mu, np.nanmean(rows_c, axis=0), rtol=1e-12)
    np.testing.assert_allclose(mc.cov, np.cov(rows_c[1:], rowvar=False, ddof=1), rtol=1e-9, atol=1e-15)
    with pytest.raises(ValueError, match="at least two sharp blocks"):
        grading.NiqeModel.fit([_hand_sums([10.0, 1.0], [0.5, 0.6])])


def test_niqe_grader(caplog):
    """frame 1 has a value for "out" only ("in" is an untouched row), frame 2 for both: each mean is over the frames with a value"""
    caplog.set_level(logging.INFO)
    m = _model(3)
    tab = grading.MetricTable(None, 64)
    g = grading.NiqeGrader(tab, None, m, ("out", "in"))
    assert tab.width == {torch.int64: 76, torch.float64: 1476}
    rng = np.random.default_rng(4)
    fa, fb = _frame_numbers(rng.standard_normal((6, 36)) + 1.0), _frame_numbers(rng.standard_normal((6, 36)) + 2.0)
    (oi, of), (ii, if_) = g.cols["out"], g.cols["in"]
    rows = [_row(tab, [("i", oi, fa[0]), ("f", of, fa[1])]), _row(tab, [("i", oi, fb[0]), ("f", of, fb[1]), ("i", ii, fa[0]), ("f", if_, fa[1])])]
    recs = [{"frame": 0, "cut": False}, {"frame": 1, "cut": False}]
    for n, (rec, (ri, rf)) in enumerate(zip(recs, rows), 1):
        g.read(n, rec, ri, rf)
    va, vb = grading.niqe_value(*fa, m), grading.niqe_value(*fb, m)
    assert recs[0]["niqe"] == {"out": va, "in": None, "gt": None, "valid_blocks": {"out": 6, "in": 0}}
    assert recs[1]["niqe"] == {"out": vb, "in": va, "gt": None, "valid_blocks": {"out": 6, "in": 6}}
    assert _messages(caplog) == ["NUM: 1, NIQE out: %.4f, in: null" % va, "NUM: 2, NIQE out: %.4f, in: %.4f" % (vb, va)]
    caplog.clear()
    result = _result(2, niqe=None)
    g.blocks = [2, 3]
    g.summary(result)
    assert list(result) == list(_result(2, niqe=None))
    assert result["niqe"] == {"model": "m", "blocks": [2, 3], "graded": "denoise", "out": (va + vb) / 2, "in": va, "gt": None,
                              "frames_with_value": {"out": 2, "in": 1}}
    assert _messages(caplog) == ["NIQE (2 frames, model m): out: %.4f, in: %.4f" % ((va + vb) / 2, va)]


# ----------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def runs(tmp_path_factory, synth):
    """the clean clip and its model, the low clip, and evals.py on it with and without --niqe; run once for the tests below"""
    d = tmp_path_factory.mktemp("niqe")
    head = _y4m().Header(NW, NH, "25:1", "p", None, "420mpeg2", "LIMITED")
    fmt = head.format("bt709")
    frames = [(t, 2) for t in range(FRAMES)]
    clean = _write(d / "clean.y4m", head, _payloads(synth, fmt, frames, True))
    low = _write(d / "low.y4m", head, _payloads(synth, fmt, frames, False))
    model = d / "model.npz"
    fit = _run("tools/niqe_fit.py", "--y4m", clean, "--out", model)
    common = ("--model_pretrain", _weights(d, synth), "--graph", "1", "--precision", "bf16", "--of_scale", "1", "--y4m_in", low, "--noref", "1")
    r = _run("evals.py", *common, "--save", d / "ev", "--y4m_frames_json", d / "frames.json", "--niqe", model)
    _run("evals.py", *common, "--save", d / "ev0", "--y4m_frames_json", d / "frames0.json")
    load = lambda p: json.load(open(str(p)))
    return types.SimpleNamespace(dir=d, fmt=fmt, frames=frames, clean=clean, low=low, model=model, fit=fit, stdout=r.stdout,
                                 m=load(d / "ev" / "Metrics.json"), rec=load(d / "frames.json"), m0=load(d / "ev0" / "Metrics.json"),
                                 rec0=load(d / "frames0.json"))


@pytest.mark.gpu
def test_evals_niqe_end_to_end(runs):
    m, rec = runs.m, runs.rec
    print(runs.fit.stdout, m["niqe"])
    assert "model.npz: 4 frames of 288x192" in runs.fit.stdout
    assert "niqe" not in runs.m0 and all("niqe" not in f for f in runs.rec0)
    assert {k: v for k, v in m.items() if k != "niqe"} == runs.m0 and list(m)[-1] == "niqe"
    assert [{k: v for k, v in f.items() if k != "niqe"} for f in rec] == runs.rec0
    nq = m["niqe"]
    assert list(nq) == ["model", "blocks", "graded", "out", "in", "gt", "frames_with_value"]
    assert nq["model"] == "model.npz" and nq["blocks"] == [2, 3] and nq["graded"] == "denoise" and nq["gt"] is None
    assert nq["frames_with_value"] == {"out": FRAMES, "in": FRAMES} and len(rec) == FRAMES
    for f in rec:
        assert list(f["niqe"]) == ["out", "in", "gt", "valid_blocks"] and f["niqe"]["gt"] is None
        assert set(f["niqe"]["valid_blocks"]) == {"out", "in"} and all(2 <= v <= 6 for v in f["niqe"]["valid_blocks"].values())
        assert all(isinstance(f["niqe"][w], float) and math.isfinite(f["niqe"][w]) and f["niqe"][w] > 0.0 for w in ("out", "in"))
    for w in ("out", "in"):
        assert nq[w] == sum(f["niqe"][w] for f in rec) / FRAMES
    lines = [line.split(" ", 3)[-1] for line in runs.stdout.split("\n")]
    assert sum(line.startswith("NUM: %d, NIQE out: " % FRAMES) for line in lines) == 1, runs.stdout[-2000:]
    assert sum(line.startswith("NIQE (%d frames, model model.npz): out: " % FRAMES) for line in lines) == 1


@pytest.mark.gpu
def test_in_is_utils_niqe_of_the_decoded_frame(runs, synth, hip_ops):
    """ "in" of every record against `utils.niqe` of the same payload decoded here, bit for bit; and the ordering: the clean clip
    against its own model scores lower than the same frames with seeded Gaussian noise added"""
    ops, dev = hip_ops
    evals = importlib.import_module("evals")
    model = grading.NiqeModel.load(str(runs.model))
    for f, p in zip(runs.rec, _payloads(synth, runs.fmt, runs.frames, False)):
        x = ops.yuv_to_planar_f32(torch.from_numpy(p.copy()).to(dev), runs.fmt)
        assert evals.utils.niqe(x, model) == f["niqe"]["in"]
        assert evals.utils.niqe(x, str(runs.model)) == f["niqe"]["in"]
    gen = torch.Generator().manual_seed(9)
    for p in _payloads(synth, runs.fmt, runs.frames, True):
        x = ops.yuv_to_planar_f32(torch.from_numpy(p.copy()).to(dev), runs.fmt)
        noisy = (x + (0.05 * torch.randn(x.shape, generator=gen)).to(dev)).clamp_(0.0, 1.0)
        a, b = evals.utils.niqe(x, model), evals.utils.niqe(noisy, model)
        print("clean %.4f, with noise %.4f" % (a, b))
        assert a < b


@pytest.mark.gpu
def test_small_frames_give_null(hip_ops):
    """a frame with fewer than two whole blocks is not graded: no launch, no value, no error"""
    ops, dev = hip_ops
    evals = importlib.import_module("evals")
    m = _model(5)
    tab = grading.MetricTable(dev, 2)
    g = grading.NiqeGrader(tab, ops, m, ("out", "in"))
    tab.build()
    x = torch.rand((1, 3, 128, 160), device=dev)
    before = dict(ops.lib.calls)
    ri, rf = tab.row(0)
    g.launch(types.SimpleNamespace(step=types.SimpleNamespace(x=x), output=x, gt=None), ri, rf)
    assert dict(ops.lib.calls) == before and g.blocks == [1, 1]
    rec = {}
    g.read(1, rec, ri.tolist(), rf.tolist())
    assert rec["niqe"] == {"out": None, "in": None, "gt": None, "valid_blocks": {"out": 0, "in": 0}}
    assert evals.utils.niqe(x, m) is None and evals.utils.niqe(x[:, :, :95], m) is None


@pytest.mark.gpu
def test_evals_niqe_dataset_mode(tmp_path, synth):
    """the PNG loop with two pairs: "out" and "gt" are the means of `utils.niqe` over the pairs, "in" is null; the ground truth's
    numbers are recomputed here from the files"""
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
    model = _model(7)
    model.save(str(tmp_path / "hand.npz"))
    r = _run("evals.py", "--dataset", "RLV", "--lowlight_images_path", data, "--model_pretrain", _weights(tmp_path, synth), "--hist_match", "0",
             "--save_images", "0", "--save", tmp_path / "ev", "--niqe", tmp_path / "hand.npz")
    m = json.load(open(str(tmp_path / "ev" / "Metrics.json")))
    print(m["niqe"])
    nq = m["niqe"]
    assert set(nq) == {"model", "blocks", "graded", "out", "in", "gt", "frames_with_value"} and "color" not in m
    assert nq["model"] == "hand.npz" and nq["blocks"] == [11, 20] and nq["graded"] == "denoise" and nq["in"] is None
    assert nq["frames_with_value"] == {"out": 2, "gt": 2} and math.isfinite(nq["out"]) and nq["out"] > 0.0
    dev = torch.device("cuda", 0)
    want = [evals.utils.niqe(evals.utils.ingest_frame(torch.from_numpy(np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8).copy()), dev),
                             grading.NiqeModel.load(str(tmp_path / "hand.npz"))) for p in paths]
    assert nq["gt"] == (want[0] + want[1]) / 2
    assert "NUM: 2, NIQE gt: " in r.stdout and "NIQE (2 images, model hand.npz): out: " in r.stdout
