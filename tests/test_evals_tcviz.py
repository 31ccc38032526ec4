"""evals.py --tc_viz / --tc_viz_max / --tc_viz_gain / --tc_flo_dir: the argument checks on the CPU; on the MI355X the
script end to end on the 128 x 160 clip of test_evals_tc.py (six frames, one scene cut, --of_scale 1): the pictures and the .flo
files are written, and everything the run reports besides is what the same run reports without the flags."""
import importlib
import json
import os

import numpy as np
import pytest

from test_evals_tc import _clip
from test_evals_y4m import H, W, THRESHOLD, _frames_of, _run, _y4m

_Y4M = ("--y4m_in", "LOW", "--y4m_gt", "GT", "--graph", "1")
_TC = _Y4M + ("--tc", "1")


@pytest.mark.parametrize("extra,words", [
    (_Y4M + ("--tc_viz", "V"), ("--tc_viz needs --tc 1",)),
    (_Y4M + ("--tc_viz_max", "2"), ("--tc_viz_max needs --tc 1",)),
    (_Y4M + ("--tc_viz_gain", "2"), ("--tc_viz_gain needs --tc 1",)),
    (_Y4M + ("--tc_flo_dir", "D"), ("--tc_flo_dir needs --tc 1",)),
    (_Y4M + ("--tc", "0", "--tc_viz", "V"), ("--tc_viz needs --tc 1",)),
    (_TC + ("--tc_viz_max", "2"), ("--tc_viz_max needs --tc_viz",)),
    (_TC + ("--tc_viz_gain", "2"), ("--tc_viz_gain needs --tc_viz",)),
    (_TC + ("--tc_flo_dir", "D", "--tc_viz_gain", "2"), ("--tc_viz_gain needs --tc_viz",)),
    (_TC + ("--tc_viz", "V", "--tc_viz_max", "-1"), ("--tc_viz_max is a flow length in pixels >= 0", "got -1")),
    (_TC + ("--tc_viz", "V", "--tc_viz_max", "nan"), ("--tc_viz_max is a flow length in pixels >= 0", "got nan")),
    (_TC + ("--tc_viz", "V", "--tc_viz_gain", "-0.5"), ("--tc_viz_gain is a factor >= 0", "got -0.5")),
    (_TC + ("--tc_viz", "V", "--y4m_out", "V"), ("--tc_viz", "is the file of --y4m_out")),
    (_TC + ("--tc_viz", "LOW"), ("--tc_viz", "is the file of --y4m_in")),
    (_TC + ("--tc_viz", "GT"), ("--tc_viz", "is the file of --y4m_gt")),
    (_TC + ("--tc_viz", "-"), ("--tc_viz must be a file",)),
], ids=["viz-alone", "max-alone", "gain-alone", "flo-alone", "viz-tc0", "max-no-viz", "gain-no-viz", "gain-flo-only", "max-negative",
        "max-nan", "gain-negative", "viz-is-out", "viz-is-in", "viz-is-gt", "viz-stdout"])
def test_tcviz_argument_checks(tmp_path, extra, words):
    """every rule is a parser error that names the flag, before anything touches the device and before --save is created"""
    for name in ("LOW", "GT"):
        (tmp_path / name).write_bytes(b"")
    extra = [str(tmp_path / a) if a in ("LOW", "GT", "V", "D") else a for a in extra]
    r = _run("evals.py", "--save", tmp_path / "out", *extra, ok=False)
    assert r.returncode == 2, (r.returncode, r.stderr[-800:])
    for w in words:
        assert w in r.stderr, (w, r.stderr[-800:])
    assert not (tmp_path / "out").exists() and not (tmp_path / "V").exists() and not (tmp_path / "D").exists()


def _white(fmt):
    """white in the stream's Y'CbCr, from the host encoder: (Y, Cb, Cr)"""
    y4m = _y4m()
    small = fmt._replace(W=2, H=2)
    y, u, v = small.planes(y4m.encode_host(np.full((2, 2, 3), 255, np.uint8), small))
    return int(y[0, 0]), int(u[0, 0]), int(v[0, 0])


@pytest.mark.gpu
def test_evals_tcviz_end_to_end(tmp_path, synth):
    FRAMES, CUT = 6, 3
    flowio = importlib.import_module("zero-tig_amd.flowio")
    common = _clip(tmp_path, synth, [(t, 2 if t < CUT else 7) for t in range(FRAMES)]) + ("--y4m_scene_cut", THRESHOLD, "--tc", "1")
    viz, flo = tmp_path / "v.y4m", tmp_path / "flo"
    out = {}
    for name, extra in (("plain", ()), ("viz", ("--tc_viz", viz, "--tc_flo_dir", flo))):
        fj, tj = tmp_path / (name + "_frames.json"), tmp_path / (name + "_timing.json")
        _run("evals.py", *common, "--save", tmp_path / name, "--y4m_frames_json", fj, "--timing_json", tj, *extra)
        out[name] = [json.load(open(str(p))) for p in (tmp_path / name / "Metrics.json", fj, tj)]
    (m0, rec0, t0), (m, rec, t) = out["plain"], out["viz"]
    # ---- the flags add two keys and change nothing else
    te = dict(m["temporal"])
    assert te.pop("viz") == {"path": str(viz), "size": [2 * W, 2 * H], "max": 0.0, "gain": 4.0} and te.pop("flo_dir") == str(flo)
    assert "viz" not in m0["temporal"] and "flo_dir" not in m0["temporal"]
    assert dict(m, temporal=te) == m0 and rec == rec0
    assert "viz" not in t0 and set(t) - set(t0) == {"viz"} and t["viz"]["viz_ms"] > 0
    # ---- the pictures
    head, pics = _frames_of(viz)
    assert (head.W, head.H, head.ctag, head.fps, head.color_range) == (2 * W, 2 * H, "420mpeg2", "25:1", "LIMITED") and len(pics) == FRAMES
    fmt = head.format("bt709")
    wy, wu, wv = _white(fmt)
    for k, p in enumerate(pics):
        y, u, v = fmt.planes(p)
        top_white = (y[:H] == wy).all() and (u[:H // 2] == wu).all() and (v[:H // 2] == wv).all()
        assert top_white == (k in (0, CUT)), k           # no partner: zero flow is white; a pair's flows are not zero everywhere
        if k in (0, CUT):
            assert (y[H:, W:] == y[H, W]).all() and y[H, W] < 20          # no error panel either: black
        assert y[H:, :W].std() > 0                                        # the frame itself
    # ---- the .flo files: two per graded pair, numbered by the current frame
    want = sorted("%06d_%s.flo" % (k, d) for k in range(FRAMES) if k not in (0, CUT) for d in ("bwd", "fwd"))
    assert sorted(os.listdir(str(flo))) == want and len(want) == 2 * 4
    flows = {n: flowio.read_flo(str(flo / n)) for n in want}
    assert all(f.shape == (H, W, 2) and f.dtype == np.float32 and np.isfinite(f).all() for f in flows.values())
    assert not np.array_equal(flows["000001_bwd.flo"], flows["000001_fwd.flo"])


@pytest.mark.gpu
def test_evals_tcviz_fixed_scale_noref(tmp_path, synth):
    """--tc_viz_max 4 --noref 1: the picture is drawn from the pair the flows come from, at a fixed scale"""
    common = _clip(tmp_path, synth, [(t, 2) for t in range(3)])
    common = common[:common.index("--y4m_gt")]              # --noref 1 takes no ground truth
    viz = tmp_path / "v.y4m"
    _run("evals.py", *common, "--save", tmp_path / "ev", "--tc", "1", "--noref", "1", "--tc_viz", viz, "--tc_viz_max", "4",
         "--tc_viz_gain", "2")
    m = json.load(open(str(tmp_path / "ev" / "Metrics.json")))
    assert m["temporal"]["viz"] == {"path": str(viz), "size": [2 * W, 2 * H], "max": 4.0, "gain": 2.0}
    assert m["temporal"]["flow_from"] == "output" and "flo_dir" not in m["temporal"]
    head, pics = _frames_of(viz)
    assert (head.W, head.H) == (2 * W, 2 * H) and len(pics) == 3


@pytest.mark.gpu
def test_evals_tcviz_too_small_for_raft(tmp_path, synth):
    """128 x 160 at --tc_scale 3 is 42 x 53: temporal is off, neither the stream nor the directory is created, one line says so"""
    common = _clip(tmp_path, synth, [(t, 2) for t in range(3)])
    viz, flo = tmp_path / "v.y4m", tmp_path / "flo"
    r = _run("evals.py", *common, "--save", tmp_path / "ev", "--hist_match", "0", "--tc", "1", "--tc_scale", "3", "--tc_viz", viz,
             "--tc_flo_dir", flo)
    m = json.load(open(str(tmp_path / "ev" / "Metrics.json")))
    assert m["temporal"] is None and m["images"] == 3
    assert not viz.exists() and not flo.exists()
    assert sum("temporal pictures off" in line for line in r.stdout.split("\n")) == 1, r.stdout[-2000:]
