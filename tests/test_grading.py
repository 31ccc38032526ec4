"""The host code under evals.py's video mode (zero-tig_amd/grading.py, zero-tig_amd/videorun.py): on the CPU the size parser, the
sequence walk against a scripted detector, the stream closer and every grader's `read` / `summary` on rows written out here; on
the MI355X the two-slot metric table past its first chunk, and the whole video mode at a chunk of 2 against a chunk of 64."""
import importlib
import json
import logging
import types

import pytest
import torch

from test_evals_tc import _clip
from test_evals_y4m import THRESHOLD

grading = importlib.import_module("zero-tig_amd.grading")
videorun = importlib.import_module("zero-tig_amd.videorun")
INF, NS = float("inf"), types.SimpleNamespace


# ------------------------------------------------------------------------------------------------------------ videorun
def test_parse_size():
    assert videorun.parse_size("1920x1080") == (1920, 1080) and videorun.parse_size("1920X1080") == (1920, 1080)
    for text in ("1920", "axb", "0x5", "1x2x3", ""):
        assert videorun.parse_size(text) is None, text


class ScriptedDetector:
    def __init__(self, verdicts):
        self.verdicts, self.pushed = list(verdicts), []

    def push(self, payload):
        self.pushed.append(payload)

    def pop(self):
        return self.verdicts[len(self.pushed) - 1]


VERDICTS = [(t in (0, 3), 0.125 * t, 0.5 * t) for t in range(6)]


def _messages(caplog):
    return [r.getMessage() for r in caplog.records]


@pytest.mark.parametrize("first,log,lines", [(0, True, ["scene cut at frame 3: score 0.3750 (rel 1.5000) > 0.04"]),
                                             (10, True, ["scene cut at frame 13: score 0.3750 (rel 1.5000) > 0.04"]), (0, False, [])],
                         ids=["first0", "first10", "silent"])
def test_sequences_with_a_scripted_detector(caplog, first, log, lines):
    caplog.set_level(logging.INFO)
    det = ScriptedDetector(VERDICTS)
    seq = videorun.Sequences(det, 0.04, first=first, log=log)
    assert [seq.next("payload%d" % t) for t in range(6)] == [True, False, False, True, False, False]
    assert det.pushed == ["payload%d" % t for t in range(6)]
    assert seq.cuts == [first + 3]                          # the detector's verdict on frame 0 is not a cut
    assert seq.scores == [0.0, 0.125, 0.25, 0.375, 0.5, 0.625] and seq.rels == [0.0, 0.5, 1.0, 1.5, 2.0, 2.5]
    assert seq.flags == [False, False, False, True, False, False]
    assert _messages(caplog) == lines
    assert seq.cuts_json() == {"threshold": 0.04, "cuts": [first + 3], "score": seq.scores, "rel": seq.rels}
    assert list(seq.cuts_json()) == ["threshold", "cuts", "score", "rel"]


def test_sequences_without_a_detector(caplog):
    caplog.set_level(logging.INFO)
    seq = videorun.Sequences(None, 0.0)
    assert [seq.next(None) for _ in range(6)] == [True, False, False, False, False, False]
    assert (seq.cuts, seq.scores, seq.rels, seq.flags) == ([], [], [], [False] * 6) and _messages(caplog) == []


class Stream:
    def __init__(self, log, name, fails=False):
        self.log, self.name, self.fails = log, name, fails

    def close(self):
        self.log.append(self.name)
        if self.fails:
            raise OSError(self.name)


def test_close_streams():
    log = []

    def streams(*fails):
        return [Stream(log, "w0", "w0" in fails), None, Stream(log, "w1", "w1" in fails), Stream(log, "w2")], [Stream(log, "r0"), None]
    videorun.close_streams(*streams())
    assert log == ["w0", "w1", "w2", "r0"]
    del log[:]
    with pytest.raises(OSError, match="w0"):                # the first failure, after everything has been closed
        videorun.close_streams(*streams("w0", "w1"))
    assert log == ["w0", "w1", "w2", "r0"]
    del log[:]
    with pytest.raises(KeyError):                           # an exception on its way out of the loop is not replaced
        try:
            raise KeyError("the loop's")
        finally:
            videorun.close_streams(*streams("w1"))
    assert log == ["w0", "w1", "w2", "r0"]


# ------------------------------------------------------------------------------------------------------------ graders, host side
def _row(tab, cells):
    """a read-back row of `tab` as the two lists a grader's `read` gets: cells = [(half, column, values)], zero elsewhere"""
    ri, rf = [0] * tab.width[torch.int64], [0.0] * tab.width[torch.float64]
    for half, column, values in cells:
        (ri if half == "i" else rf)[column] = values
    return ri, rf


def _result(images, **more):
    r = dict.fromkeys(("Total_PSNR", "Total_SSIM", "Total_LPIPS", "Total_PSNR_HM", "Total_SSIM_HM", "Total_LPIPS_HM"))
    return dict(r, images=images, planes=None, **more)


def test_rgb_grader_with_lpips_and_hist_match(caplog):
    """12 samples: a squared error of 7803 is 255^2 * 12 / 100, PSNR 20; of 78030, PSNR 10; of 0, inf.  The LPIPS layers of frame 1
    add up to 2 from left to right ((1e16 + 1) - 1e16 = 0) and to 3 in exact arithmetic."""
    caplog.set_level(logging.INFO)
    tab = grading.MetricTable(None, 64)
    g = grading.RgbGrader(tab, None, 12, hist_match=lambda a, b: a, lpips=object())
    p, hm = g.passes
    rows = [_row(tab, [("i", p.sq, [0]), ("f", p.ssim, [0.5]), ("f", p.lpips, [1e16, 1.0, -1e16, 1.0, 1.0]),
                       ("i", hm.sq, [7803]), ("f", hm.ssim, [0.25]), ("f", hm.lpips, [0.5, 0.0, 0.0, 0.0, 0.0])]),
            _row(tab, [("i", p.sq, [7803]), ("f", p.ssim, [1.0]), ("f", p.lpips, [0.25, 0.0, 0.0, 0.0, 0.0]),
                       ("i", hm.sq, [78030]), ("f", hm.ssim, [0.75]), ("f", hm.lpips, [1.5, 0.0, 0.0, 0.0, 0.0])])]
    recs = [{"frame": 0, "cut": False}, {"frame": 1, "cut": True}]
    for n, (rec, (ri, rf)) in enumerate(zip(recs, rows), 1):
        g.read(n, rec, ri, rf)
    assert recs == [{"frame": 0, "cut": False, "PSNR": INF, "SSIM": 0.5, "LPIPS": 2.0, "PSNR_HM": 20.0, "SSIM_HM": 0.25, "LPIPS_HM": 0.5},
                    {"frame": 1, "cut": True, "PSNR": 20.0, "SSIM": 1.0, "LPIPS": 0.25, "PSNR_HM": 10.0, "SSIM_HM": 0.75, "LPIPS_HM": 1.5}]
    assert list(recs[0]) == ["frame", "cut", "PSNR", "SSIM", "LPIPS", "PSNR_HM", "SSIM_HM", "LPIPS_HM"]
    assert _messages(caplog) == [
        "NUM: 1, PSNR: inf, SSIM: 0.500, LPIPS: 2.000", "Total PSNR: inf, Total SSIM: 0.500, Total LPIPS: 2.000",
        "NUM: 1, PSNR_HM: 20.000, SSIM_HM: 0.250, LPIPS_HM: 0.500", "Total PSNR_HM: 20.000, Total SSIM_HM: 0.250, Total LPIPS_HM: 0.500",
        "NUM: 2, PSNR: 20.000, SSIM: 1.000, LPIPS: 0.250", "Total PSNR: inf, Total SSIM: 0.750, Total LPIPS: 1.125",
        "NUM: 2, PSNR_HM: 10.000, SSIM_HM: 0.750, LPIPS_HM: 1.500", "Total PSNR_HM: 15.000, Total SSIM_HM: 0.500, Total LPIPS_HM: 1.000"]
    result = _result(2)
    g.summary(result)
    assert result == {"Total_PSNR": INF, "Total_SSIM": 0.75, "Total_LPIPS": 1.125, "Total_PSNR_HM": 15.0, "Total_SSIM_HM": 0.5,
                      "Total_LPIPS_HM": 1.0, "images": 2, "planes": None}
    assert list(result) == list(_result(2))


def test_rgb_grader_alone(caplog):
    caplog.set_level(logging.INFO)
    tab = grading.MetricTable(None, 64)
    g = grading.RgbGrader(tab, None, 12)
    p, = g.passes
    assert p.lpips is None
    rec = {"frame": 0, "cut": False}
    g.read(1, rec, *_row(tab, [("i", p.sq, [78030]), ("f", p.ssim, [-0.25])]))
    assert rec == {"frame": 0, "cut": False, "PSNR": 10.0, "SSIM": -0.25} and list(rec) == ["frame", "cut", "PSNR", "SSIM"]
    assert _messages(caplog) == ["NUM: 1, PSNR: 10.000, SSIM: -0.250", "Total PSNR: 10.000, Total SSIM: -0.250"]
    result = _result(1)
    g.summary(result)
    assert result == dict(_result(1), Total_PSNR=10.0, Total_SSIM=-0.25)
    empty = _result(0)                                      # no frame at all: the sums over one
    grading.RgbGrader(grading.MetricTable(None, 64), None, 12).summary(empty)
    assert empty == dict(_result(0), Total_PSNR=0.0, Total_SSIM=0.0)


def test_plane_grader(caplog):
    """8-bit 4 x 4 luma, 2 x 2 chroma: an SSE of 10404 is 255^2 * 16 / 100 and one of 2601 is 255^2 * 4 / 100, PSNR 20; an SSE of 0
    has no PSNR"""
    caplog.set_level(logging.INFO)
    tab = grading.MetricTable(None, 64)
    g = grading.PlaneGrader(tab, None, NS(H=4, W=4, chroma_shape=(2, 2), depth=8, ss=420))
    rec = {"frame": 0, "cut": False}
    g.read(1, rec, *_row(tab, [("i", g.sse, [10404, 0, 2601])] + [("f", c, [v]) for c, v in zip(g.ssim, (0.5, 0.25, 1.0))]))
    assert rec == {"frame": 0, "cut": False, "SSE": [10404, 0, 2601], "SSIM_Y": 0.5, "SSIM_U": 0.25, "SSIM_V": 1.0}
    assert list(rec) == ["frame", "cut", "SSE", "SSIM_Y", "SSIM_U", "SSIM_V"]
    assert _messages(caplog) == ["NUM: 1, SSE_Y: 10404, SSE_U: 0, SSE_V: 2601, SSIM_Y: 0.500, SSIM_U: 0.250, SSIM_V: 1.000"]
    result = _result(1)
    g.summary(result)
    assert result["planes"] == {"depth": 8, "ss": 420, "samples": [16, 4, 4], "SSE": [10404, 0, 2601], "PSNR_Y": 20.0, "PSNR_U": None,
                                "PSNR_V": 20.0, "SSIM_Y": 0.5, "SSIM_U": 0.25, "SSIM_V": 1.0}
    assert list(result["planes"]) == ["depth", "ss", "samples", "SSE", "PSNR_Y", "PSNR_U", "PSNR_V", "SSIM_Y", "SSIM_U", "SSIM_V"]


def test_plane_grader_off(caplog):
    caplog.set_level(logging.INFO)
    tab = grading.MetricTable(None, 64)
    g = grading.PlaneGrader(tab, None, None)
    assert tab.width == {torch.int64: 0, torch.float64: 0}
    rec = {"frame": 0, "cut": False}
    g.read(1, rec, [], [])
    assert rec == {"frame": 0, "cut": False, "SSE": None, "SSIM_Y": None, "SSIM_U": None, "SSIM_V": None}
    result = _result(1)
    g.summary(result)
    assert result == _result(1) and _messages(caplog) == []


TC = NS(h=2, w=5)                                           # 10 pixels: MABD = sum / 30
TE_KEYS = ["scale", "size", "pairs", "raft", "valid_share", "E_warp", "E_static", "MABD", "E_warp_gt", "E_static_gt", "MABD_gt", "MABD_mse"]


def _temporal_grader(from_output, flags, extra=None):
    tab = grading.MetricTable(None, 64)
    g = grading.TemporalGrader(tab, TC, from_output, {"scale": 2, "raft": "checkpoint"}, extra or {})
    g.flags = list(flags)                                   # what `launch` records: tc.push's return value per frame
    return tab, g


def test_temporal_grader(caplog):
    caplog.set_level(logging.INFO)
    tab, g = _temporal_grader(False, [False, True, True], {"flo_dir": "D"})
    rows = [_row(tab, [("i", g.n, [77, 77]), ("f", g.sums, [9.0] * 6)]),       # the first frame of a sequence: a stale row, not read
            _row(tab, [("i", g.n, [4, 4]), ("f", g.sums, [6.0, 3.0, 15.0, 1.5, 0.75, 7.5])]),
            _row(tab, [("i", g.n, [0, 0]), ("f", g.sums, [0.0, 3.0, 15.0, 0.0, 0.75, 7.5])])]
    recs = [{"frame": t, "cut": False} for t in range(3)]
    for n, (rec, (ri, rf)) in enumerate(zip(recs, rows), 1):
        g.read(n, rec, ri, rf)
    assert recs == [{"frame": 0, "cut": False, "TC": None},
                    {"frame": 1, "cut": False, "TC": {"N": 4, "out": [6.0, 3.0, 15.0], "gt": [1.5, 0.75, 7.5]}},
                    {"frame": 2, "cut": False, "TC": {"N": 0, "out": [0.0, 3.0, 15.0], "gt": [0.0, 0.75, 7.5]}}]
    assert _messages(caplog) == ["NUM: 2, TC valid: 4, E_warp: 0.500000 (gt 0.125000), MABD: 0.500000 (gt 0.250000)",
                                 "NUM: 3, TC valid: 0, E_warp: nan (gt nan), MABD: 0.500000 (gt 0.250000)"]
    caplog.clear()
    result = _result(3, temporal=None)
    g.summary(result)
    assert result["temporal"] == {"scale": 2, "size": [5, 2], "pairs": 2, "raft": "checkpoint", "valid_share": 0.2, "E_warp": 0.5,
                                  "E_static": 0.1, "MABD": 0.5, "E_warp_gt": 0.125, "E_static_gt": 0.025, "MABD_gt": 0.25,
                                  "MABD_mse": 0.0625, "flo_dir": "D"}
    assert list(result["temporal"]) == TE_KEYS + ["flo_dir"]
    assert _messages(caplog) == ["temporal (scale 2, 2 pairs): valid_share: 0.2, E_warp: 0.5, E_warp_gt: 0.125, E_static: 0.1, "
                                 "E_static_gt: 0.025, MABD: 0.5, MABD_gt: 0.25, MABD_mse: 0.0625"]


def test_temporal_grader_no_valid_pixel(caplog):
    caplog.set_level(logging.INFO)
    tab, g = _temporal_grader(False, [False, True])
    g.read(2, {}, *_row(tab, [("i", g.n, [0, 0]), ("f", g.sums, [0.0, 3.0, 15.0, 0.0, 0.75, 7.5])]))
    caplog.clear()
    result = _result(2, temporal=None)
    g.summary(result)
    assert result["temporal"] == {"scale": 2, "size": [5, 2], "pairs": 1, "raft": "checkpoint", "valid_share": 0.0, "E_warp": None,
                                  "E_static": 0.1, "MABD": 0.5, "E_warp_gt": None, "E_static_gt": 0.025, "MABD_gt": 0.25, "MABD_mse": 0.0625}
    assert _messages(caplog) == ["temporal (scale 2, 1 pairs): valid_share: 0, E_warp: null, E_warp_gt: null, E_static: 0.1, "
                                 "E_static_gt: 0.025, MABD: 0.5, MABD_gt: 0.25, MABD_mse: 0.0625"]


def test_temporal_grader_flows_from_the_output(caplog):
    caplog.set_level(logging.INFO)
    tab, g = _temporal_grader(True, [False, True])
    recs = [{}, {}]
    g.read(1, recs[0], *_row(tab, []))
    g.read(2, recs[1], *_row(tab, [("i", g.n, [4, 4]), ("f", g.sums, [6.0, 3.0, 15.0, 6.0, 3.0, 15.0])]))
    assert recs == [{"TC": None}, {"TC": {"N": 4, "out": [6.0, 3.0, 15.0], "gt": None}}]
    result = _result(2, noref=None, temporal=None)
    g.summary(result)
    assert result["temporal"] == {"scale": 2, "size": [5, 2], "pairs": 1, "raft": "checkpoint", "valid_share": 0.4, "E_warp": 0.5,
                                  "E_static": 0.1, "MABD": 0.5, "E_warp_gt": None, "E_static_gt": None, "MABD_gt": None, "MABD_mse": None,
                                  "flow_from": "output"}
    assert list(result["temporal"]) == TE_KEYS + ["flow_from"]
    assert _messages(caplog) == ["NUM: 2, TC valid: 4, E_warp: 0.500000, MABD: 0.500000 (flows from the output)",
                                 "temporal (scale 2, 1 pairs): valid_share: 0.4, E_warp: 0.5, E_warp_gt: null, E_static: 0.1, "
                                 "E_static_gt: null, MABD: 0.5, MABD_gt: null, MABD_mse: null"]


def test_temporal_grader_off(caplog):
    """the frame is too small for RAFT: no columns, every field null"""
    caplog.set_level(logging.INFO)
    tab = grading.MetricTable(None, 64)
    g = grading.TemporalGrader(tab, None, False, {"scale": 3, "raft": "checkpoint"}, {})
    assert tab.width == {torch.int64: 0, torch.float64: 0}
    g.launch(NS(cut=True), None, None)
    rec = {}
    g.read(1, rec, [], [])
    result = _result(1, temporal=None)
    g.summary(result)
    assert rec == {"TC": None} and result == _result(1, temporal=None) and _messages(caplog) == []


def test_noref_grader(caplog):
    """frame 1 has one sample (no LOE), frame 2 an input of lightness 0 (no gain).  The stream's gain is (9 + 50) / (3 + 0), not
    the mean of the frames' gains, which is 3."""
    caplog.set_level(logging.INFO)
    tab = grading.MetricTable(None, 64)
    g = grading.NorefGrader(tab, None, (50, 63))
    rows = [_row(tab, [("i", g.full, [1, 0, 3, 9, 0, 0]), ("i", g.sub, [2500, 0, 7500, 22500, 0, 0]), ("f", g.ents, [0.0, 0.0]),
                       ("f", g.ents_sub, [7.0, 7.0])]),
            _row(tab, [("i", g.full, [10, 18, 0, 50, 1, 2]), ("i", g.sub, [4, 6, 0, 20, 0, 0]), ("f", g.ents, [0.0, 1.5]),
                       ("f", g.ents_sub, [7.0, 7.0])])]
    recs = [{"frame": 0, "cut": False}, {"frame": 1, "cut": False}]
    for n, (rec, (ri, rf)) in enumerate(zip(recs, rows), 1):
        g.read(n, rec, ri, rf)
    assert recs[0] == {"frame": 0, "cut": False, "noref": {
        "LOE": None, "LOE_50": 0.0, "L_in": 3.0, "L_out": 9.0, "gain": 3.0, "entropy_in": 0.0, "entropy_out": 0.0, "sat_out": 0.0,
        "black_out": 0.0, "ints": [1, 0, 3, 9, 0, 0], "ints_50": [2500, 0, 7500, 22500, 0, 0]}}
    assert recs[1]["noref"] == {"LOE": 0.2, "LOE_50": 1.5, "L_in": 0.0, "L_out": 5.0, "gain": None, "entropy_in": 0.0, "entropy_out": 1.5,
                                "sat_out": 0.1, "black_out": 0.2, "ints": [10, 18, 0, 50, 1, 2], "ints_50": [4, 6, 0, 20, 0, 0]}
    assert list(recs[1]["noref"]) == list(grading.NR_KEYS) + ["ints", "ints_50"]
    assert _messages(caplog) == [
        "NUM: 1, LOE: null, LOE_50: 0.0000, L_in: 3.0000, L_out: 9.0000, gain: 3.0000, entropy_in: 0.0000, entropy_out: 0.0000, "
        "sat_out: 0.0000, black_out: 0.0000",
        "Total LOE: null, Total LOE_50: 0.0000, Total L_out: 9.0000, Total gain: 3.0000",
        "NUM: 2, LOE: 0.2000, LOE_50: 1.5000, L_in: 0.0000, L_out: 5.0000, gain: null, entropy_in: 0.0000, entropy_out: 1.5000, "
        "sat_out: 0.1000, black_out: 0.2000",
        "Total LOE: 0.2000, Total LOE_50: 0.7500, Total L_out: 7.0000, Total gain: 19.6667"]
    caplog.clear()
    result = _result(2, noref=None)
    g.summary(result)
    assert result["noref"] == {"graded": "denoise", "LOE": 0.2, "LOE_50": 0.75, "L_in": 1.5, "L_out": 7.0, "gain": 59 / 3, "entropy_in": 0.0,
                               "entropy_out": 0.75, "sat_out": 0.05, "black_out": 0.1}
    assert list(result["noref"]) == ["graded"] + list(grading.NR_KEYS) and list(result) == list(_result(2, noref=None))
    assert _messages(caplog) == ["no-reference (2 frames, the denoise result against the decoded input): LOE: 0.2, LOE_50: 0.75, "
                                 "L_in: 1.5, L_out: 7, gain: 19.6667, entropy_in: 0, entropy_out: 0.75, sat_out: 0.05, black_out: 0.1"]


def test_evals_keeps_the_names_tools_use():
    evals = importlib.import_module("evals")
    assert evals.loe50_grid is grading.loe50_grid and evals.noref_values is grading.noref_values and evals.NR_KEYS is grading.NR_KEYS


# ------------------------------------------------------------------------------------------------------------ on the MI355X
@pytest.mark.gpu
def test_metric_table_two_slots_one_chunk_late(hip_ops):
    """7 frames at a chunk of 2: each slot is written twice and a tail of one row is left.  After frame k the rows read are those of
    every full chunk but the newest: the read never waits for the chunk just copied."""
    dev = hip_ops[1]
    tab = grading.MetricTable(dev, 2)
    a, b, c = tab.ints("a", 1), tab.ints("b", 3), tab.floats("c", 2)
    tab.build()
    got = []
    for t in range(7):
        ri, rf = tab.row(t)
        assert tuple(ri.shape) == (4,) and tuple(rf.shape) == (2,) and ri.dtype == torch.int64 and rf.dtype == torch.float64
        ri[a].fill_(7 * t + 1)
        ri[b].copy_(torch.arange(3, device=dev) * (t + 1) + 100)
        rf[c].copy_(torch.tensor([t + 0.5, -0.25 * t], dtype=torch.float64))
        got += tab.advance(t + 1)
        assert len(got) == max(0, ((t + 1) // 2 - 1) * 2), (t, len(got))
    got += tab.finish()
    assert [n for n, _, _ in got] == list(range(7))
    for t, ri, rf in got:
        assert ri[a] == [7 * t + 1] and ri[b] == [100, 101 + t, 102 + 2 * t] and rf[c] == [t + 0.5, -0.25 * t], (t, ri, rf)
    assert tab.finish() == [] and tab.pending == []


def _video_mode(monkeypatch, tmp_path, chunk, argv):
    """evals.main_y4m in this process with evals.CHUNK = chunk -> the bytes of (Metrics.json, the frames JSON)"""
    evals = importlib.import_module("evals")
    monkeypatch.setattr(evals, "CHUNK", chunk)
    save, fj = tmp_path / ("ev%d" % chunk), tmp_path / ("frames%d.json" % chunk)
    args = evals.parser.parse_args([str(a) for a in argv + ("--save", save, "--y4m_frames_json", fj)])
    root = logging.getLogger()
    before = list(root.handlers)
    try:
        assert evals.check_y4m_args(args) is True
        evals.main_y4m(args)
    finally:                                                # main_y4m adds a FileHandler (and, first, basicConfig's) on every call
        for h in [h for h in root.handlers if h not in before]:
            root.removeHandler(h)
            h.close()
    return (save / "Metrics.json").read_bytes(), fj.read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("noref", [False, True], ids=["gt", "noref"])
def test_video_mode_is_chunk_independent(tmp_path, synth, monkeypatch, noref):
    """5 frames at CHUNK 2: slot 0 is written twice, every read but the last is one chunk late, and a tail of one frame is left;
    at CHUNK 64 the table is read once, at the end.  Both must write the same bytes."""
    argv = _clip(tmp_path, synth, [(t, 2 if t < 3 else 7) for t in range(5)]) + ("--tc", "1", "--y4m_scene_cut", THRESHOLD)
    if noref:
        argv = argv[:argv.index("--y4m_gt")] + argv[argv.index("--y4m_gt") + 2:] + ("--noref", "1")
    m64, f64 = _video_mode(monkeypatch, tmp_path, 64, argv)
    m2, f2 = _video_mode(monkeypatch, tmp_path, 2, argv)
    m, rec = json.loads(m64), json.loads(f64)
    assert m["images"] == 5 and m["cuts"] == [3] and m["temporal"]["pairs"] == 3 and ("noref" in m) == noref
    assert [f["frame"] for f in rec] == list(range(5)) and [f["TC"] is None for f in rec] == [True, False, False, True, False]
    assert m2 == m64 and f2 == f64
