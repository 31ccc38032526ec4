"""Scene cuts in a Y4M stream: the two integer kernels of zt_scene.hip against the definition restated here in numpy
int64, the host rule, `SceneCut` on synthetic clips with one cut, `InferStep` across a cut and predict.py --y4m_scene_cut.
The grid kernel is a template over the sample type; its 2-byte instantiation (deep planes) is pinned in test_y4m_deep.py.

The definition.  The luma plane Y [H][W] (the first H * W bytes of a payload) is cut into 16 x 16 cells, gh = ceil(H / 16) rows of
gw = ceil(W / 16); edge cells hold the pixels that exist.  G[i][j] = sum over the cell of max(Y - yo, 0) (uint32; yo = 16 for
limited range, 0 for full range).  For two consecutive frames sad = sum |G_n - G_(n-1)| and tot = sum (G_n + G_(n-1)), both uint64.
On the host rel_n = sad / max(tot, 1) as a Python float, rel_0 = 0, score_n = min(rel_n, |rel_n - rel_(n-1)|),
cut_n = score_n > threshold; frame 0 always starts a sequence."""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

THRESHOLD = 0.04
CUT_AT = 5                                                  # frames 0-4 from seed 2, frames 5-8 from seed 7
EXPECT_CUTS = [True, False, False, False, False, True, False, False, False]


def _y4m():
    return importlib.import_module("zero-tig_amd.y4m")


def _scenecut():
    return importlib.import_module("zero-tig_amd.scenecut")


# ------------------------------------------------------------------------------------- the definition, restated (numpy int64)
def ref_grid(plane, yo):
    H, W = plane.shape
    gh, gw = -(-H // 16), -(-W // 16)
    v = np.zeros((gh * 16, gw * 16), dtype=np.int64)        # pixels that do not exist add nothing
    v[:H, :W] = np.maximum(plane.astype(np.int64) - yo, 0)
    return v.reshape(gh, 16, gw, 16).sum(axis=(1, 3))


def ref_pair(a, b):
    a, b = a.astype(np.int64).reshape(-1), b.astype(np.int64).reshape(-1)
    return int(np.abs(a - b).sum()), int((a + b).sum())


def ref_rule(pairs, threshold):
    """[(sad, tot)] of frames 1.. -> [(is_cut, score, rel)] of frames 0.."""
    out, prev = [(True, 0.0, 0.0)], 0.0
    for sad, tot in pairs:
        rel = sad / max(tot, 1)
        score = min(rel, abs(rel - prev))
        out.append((score > threshold, score, rel))
        prev = rel
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
_PLANES = {}


def plane(H, W):
    """random luma plane holding every code 0..255 (the four codes 3, 16, 17, 255 at 2 x 2) -- made once, never modified"""
    if (H, W) not in _PLANES:
        rng = np.random.default_rng(100 * H + W)
        p = rng.integers(0, 256, H * W, dtype=np.uint8)
        if H * W >= 256:
            p[rng.permutation(H * W)[:256]] = np.arange(256, dtype=np.uint8)
            assert len(np.unique(p)) == 256
        else:
            p[:] = np.array([3, 16, 17, 255], dtype=np.uint8)
        p = p.reshape(H, W)
        p.setflags(write=False)
        _PLANES[(H, W)] = p
    return _PLANES[(H, W)]


def _aligned(a, dev, offset=0):
    """the bytes / words of `a` in a fresh device buffer, `offset` elements behind a 16-byte aligned address"""
    a = np.ascontiguousarray(a).reshape(-1)
    t = torch.from_numpy(a.copy())
    buf = torch.zeros(a.size + offset + 16, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + a.size]
    view.copy_(t)
    return view


def _fmt444(H, W, yo):
    return _y4m().YuvFormat(W, H, 444, 0, "bt709", 0 if yo else 1)


_CLIPS = {}


def clip(synth, H, W, ctag, full):
    """(fmt, 9 payloads): frames 0-4 of seed 2, then frames 5-8 of seed 7, made as tests/test_y4m.py makes its payloads"""
    key = (H, W, ctag, full)
    if key not in _CLIPS:
        y = _y4m()
        fmt = y.Header(W, H, None, None, None, ctag, full).format("bt709")
        pay = []
        for t in range(9):
            a = np.asarray(synth.lowlight_frame(t, H, W, 2 if t < CUT_AT else 7), dtype=np.float32)
            rgb = (np.transpose(a[0], (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8)
            p = y.encode_host(rgb, fmt)
            p.setflags(write=False)
            pay.append(p)
        _CLIPS[key] = (fmt, pay)
    return _CLIPS[key]


def clip_reference(fmt, pay):
    """the restatement's (is_cut, score, rel) per frame, with its own margins asserted: a change to `synth` fails here"""
    yo = 0 if fmt.full else 16
    grids = [ref_grid(fmt.planes(p)[0], yo) for p in pay]
    ref = ref_rule([ref_pair(grids[n], grids[n - 1]) for n in range(1, len(pay))], THRESHOLD)
    assert ref[CUT_AT][1] > 0.06, ref[CUT_AT]
    assert all(r[1] < 0.02 for n, r in enumerate(ref) if n != CUT_AT), [r[1] for r in ref]
    assert [r[0] for r in ref] == EXPECT_CUTS
    return ref


# --------------------------------------------------------------------------------------------------------- 1. the grid
# 2 x 2 and 16 x 16: one cell; 17 x 33: one extra row and column of cells; 38 x 52: tails in both axes; 24 x 208 and 48 x 1040: the
# 16-byte path (with a cut bottom row of cells / 65 cells per row, more than one wave's run); 270 x 480: more than one workgroup
GRID_SIZES = [(2, 2), (16, 16), (17, 33), (38, 52), (24, 208), (48, 1040), (270, 480)]


@pytest.mark.parametrize("yo", [0, 16])
def test_grid_definition(backend, yo):
    ops, dev, _ = backend
    for H, W in GRID_SIZES:
        p = plane(H, W)
        assert (p < yo).any() or yo == 0
        d = _aligned(p, dev)
        got = ops.luma_grid(d, _fmt444(H, W, yo))
        assert got.dtype == torch.int32 and tuple(got.shape) == (-(-H // 16), -(-W // 16))
        assert np.array_equal(got.cpu().numpy().astype(np.int64), ref_grid(p, yo)), (H, W)
        assert torch.equal(ops.luma_grid(d.view(H, W), _fmt444(H, W, yo)), got), (H, W)
    # the same 24 x 208 plane one byte behind an aligned address: the byte path, the same grid
    H, W = 24, 208
    d = _aligned(plane(H, W), dev, offset=1)
    assert d.data_ptr() % 16 == 1 and W % 16 == 0
    assert np.array_equal(ops.luma_grid(d, _fmt444(H, W, yo)).cpu().numpy().astype(np.int64), ref_grid(plane(H, W), yo))


def test_grid_of_a_payload(backend):
    """a whole payload goes in as it is: the grid is that of its first H * W bytes, whatever the chroma planes hold"""
    ops, dev, _ = backend
    y = _y4m()
    for ctag, full, H, W in (("420mpeg2", None, 38, 52), ("422", "FULL", 17, 48)):
        fmt = y.Header(W, H, None, None, None, ctag, full).format("bt709")
        payload = np.random.default_rng(H).integers(0, 256, fmt.frame_bytes, dtype=np.uint8)
        got = ops.luma_grid(_aligned(payload, dev), fmt).cpu().numpy().astype(np.int64)
        assert np.array_equal(got, ref_grid(fmt.planes(payload)[0], 0 if full else 16)), ctag


# --------------------------------------------------------------------------------------------------------- 2. the pair
def _pair(ops, dev, a, b, offset=0):
    out = torch.tensor([-0x0123456789ABCDEF, 0x7EDCBA9876543210], dtype=torch.int64, device=dev)    # garbage: overwritten
    res = ops.grid_sad(_aligned(a.astype(np.int32), dev, offset), _aligned(b.astype(np.int32), dev, offset), out=out)
    assert res is out
    return tuple(int(v) for v in out.cpu())


def test_pair_exact(backend):
    ops, dev, _ = backend
    rng = np.random.default_rng(11)
    for n in (1, 63, 64, 65, 8160):
        a, b = rng.integers(0, 65281, n, dtype=np.int64), rng.integers(0, 65281, n, dtype=np.int64)
        assert _pair(ops, dev, a, b) == ref_pair(a, b), n
        assert _pair(ops, dev, a, b, offset=1) == ref_pair(a, b), n           # 4-byte aligned only: the scalar loads
    n = 32400                                                                  # a 4K grid: 135 x 240 cells
    full, zero = np.full(n, 65280, dtype=np.int64), np.zeros(n, dtype=np.int64)
    assert _pair(ops, dev, full, zero) == (2115072000, 2115072000)
    assert _pair(ops, dev, full, full) == (0, 4230144000) and 2 ** 31 < 4230144000 < 2 ** 32     # 98.5 % of the uint32 range
    n = 34560                                                                  # DCI 4K (2160 x 4096): 135 x 256 cells, past 2^32
    full = np.full(n, 65280, dtype=np.int64)
    assert _pair(ops, dev, full, full) == (0, 4512153600) and 4512153600 > 2 ** 32
    assert _pair(ops, dev, full, np.zeros(n, dtype=np.int64)) == (2256076800, 2256076800)
    n, full, zero = 32400, np.full(32400, 65280, dtype=np.int64), np.zeros(32400, dtype=np.int64)
    got = ops.grid_sad(_aligned(full.astype(np.int32), dev), _aligned(zero.astype(np.int32), dev))      # out=None
    assert got.dtype == torch.int64 and got.tolist() == [2115072000, 2115072000]


# ------------------------------------------------------------------------------------------------- 3. argument errors
def test_argument_errors(backend):
    ops, dev, _ = backend
    p = torch.zeros(64, dtype=torch.uint8, device=dev)
    g = torch.zeros(64, dtype=torch.int32, device=dev)
    out = torch.zeros(2, dtype=torch.int64, device=dev)
    for H, W, yo in ((0, 4, 16), (4, 0, 16), (-1, 4, 16), (4, 4, 256), (4, 4, -1)):
        with pytest.raises(RuntimeError, match="1001"):                 # the library's own argument check
            ops.lib.call("zt_luma_grid_u8", p, H, W, yo, g, None)
    for n in (0, -3):
        with pytest.raises(RuntimeError, match="1001"):
            ops.lib.call("zt_grid_sad_u32", g, g, n, out, None)
    ops.lib.call("zt_luma_grid_u8", p, 4, 4, 255, g, None)              # the ends of the range are taken
    ops.lib.call("zt_luma_grid_u8", p, 4, 4, 0, g, None)
    fmt = _fmt444(4, 4, 16)
    with pytest.raises(AssertionError):                                 # the wrapper's checks, as for the yuv wrappers
        ops.luma_grid(p, fmt)                                           # 64 bytes are neither the plane nor the payload
    with pytest.raises(AssertionError):
        ops.luma_grid(p[:16].to(torch.int32), fmt)
    with pytest.raises(AssertionError):
        ops.grid_sad(g, g[:32])
    with pytest.raises(ValueError):
        ops.luma_grid(p, _y4m().YuvFormat(5, 4, 420, 0, "bt709", 0))


# -------------------------------------------------------------------------------------------- 4. exposure invariance
@pytest.mark.parametrize("yo", [0, 16])
def test_exposure_invariance(backend, yo):
    """doubling Y - yo doubles sad and tot exactly, so rel does not move: an exposure change is no cut"""
    ops, dev, _ = backend
    H, W = 38, 52
    rng = np.random.default_rng(7 + yo)
    A, B = (rng.integers(0, 101, (H, W)).astype(np.uint8) + np.uint8(yo) for _ in range(2))
    fmt = _fmt444(H, W, yo)

    def pair(a, b):
        ga, gb = ops.luma_grid(_aligned(a, dev), fmt), ops.luma_grid(_aligned(b, dev), fmt)
        return tuple(ops.grid_sad(ga, gb).tolist())
    sad, tot = pair(A, B)
    assert (sad, tot) == ref_pair(ref_grid(A, yo), ref_grid(B, yo)) and sad > 0
    A2, B2 = ((yo + 2 * (p.astype(np.int64) - yo)).astype(np.uint8) for p in (A, B))
    assert 200 <= int(A2.max()) <= 255
    sad2, tot2 = pair(A2, B2)
    assert (sad2, tot2) == (2 * sad, 2 * tot)
    assert sad2 / max(tot2, 1) == sad / max(tot, 1)


# ------------------------------------------------------------------------------------------------------- 5. SceneCut
@pytest.mark.parametrize("H,W,ctag,full", [(96, 128, "420mpeg2", None), (50, 70, "444", None)])
def test_scenecut_on_a_clip(backend, synth, H, W, ctag, full):
    ops, dev, name = backend
    fmt, pay = clip(synth, H, W, ctag, full)
    ref = clip_reference(fmt, pay)
    det = _scenecut().SceneCut(ops, dev, fmt, THRESHOLD)
    got = []
    for t, p in enumerate(pay):
        payload = torch.from_numpy(p.copy())
        if name == "hip":                                   # pinned host memory, or already on the device
            payload = payload.pin_memory() if t % 2 == 0 else payload.to(dev)
        det.push(payload)
        got.append(det.pop())
    assert [g[0] for g in got] == EXPECT_CUTS
    assert got == ref                                       # scores and rels are the restatement's Python floats, exactly
    assert det.frames == 9 and det.wait >= 0.0
    with pytest.raises(AssertionError):
        det.pop()                                           # nothing pushed


# ------------------------------------------------------------------------------------------- 6. the host rule alone
def test_host_rule():
    rule = _scenecut().CutRule(THRESHOLD)
    assert rule.first() == (True, 0.0, 0.0)
    # still scene; a cut; the new scene; motion setting in over three frames and then steady at rel 0.08; an all-black pair
    pairs = [(100, 10000), (120, 10000), (5000, 10000), (110, 10000), (400, 10000), (700, 10000), (800, 10000), (800, 10000),
             (1600, 20000), (800, 10000), (0, 0), (0, 0)]
    got = [rule.update(s, t) for s, t in pairs]
    ref = ref_rule(pairs, THRESHOLD)[1:]
    assert got == ref
    assert [g[0] for g in got] == [False, False, True, False, False, False, False, False, False, False, False, False]
    assert got[2][2] == 0.5 and got[2][1] == abs(0.5 - 0.012)
    assert [g[2] for g in got[6:10]] == [0.08] * 4 and [g[1] for g in got[7:10]] == [0.0] * 3      # sustained motion: no cut
    assert got[10] == (False, 0.0, 0.0) and got[11] == (False, 0.0, 0.0)                             # tot = 0 divides by 1
    assert all(0.0 <= g[2] <= 1.0 for g in got)
    # a jump INTO fast motion within one frame does read as a cut (8e): the score is the smaller of rel and its change
    rule = _scenecut().CutRule(THRESHOLD)
    rule.first()
    assert rule.update(100, 10000)[0] is False and rule.update(800, 10000)[0] is True and rule.update(800, 10000)[0] is False


# ------------------------------------------------------------------------------------------- 7. InferStep across a cut
def _net(ops, dev, synth, precision, seed=1):
    net_mod = importlib.import_module("zero-tig_amd.network")
    net = net_mod.Finetunemodel(argparse.Namespace(dataset="RLV", of_scale=1), ops=ops, precision=precision)
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(seed).items()})
    return net.to(dev).eval()


def _keep(step):
    return [step.out[0].clone(), step.out[1].clone(), step.yuv[0].clone(), step.yuv[1].clone()]


@pytest.mark.gpu
def test_inferstep_across_a_cut(hip_ops, synth):
    """A: the 9-frame clip through SceneCut + a graph-replayed InferStep; B: a fresh step fed frames 5-8 alone; C: the clip without
    the detector.  After the cut A is B bit for bit (the cache restarted), C is not (it warped the old scene in), and the graph
    captured before the cut keeps serving the frames after it."""
    ops, dev = hip_ops
    infer = importlib.import_module("zero-tig_amd.infer")
    fmt, pay = clip(synth, 128, 160, "420mpeg2", None)
    clip_reference(fmt, pay)
    pinned = [torch.from_numpy(p.copy()).pin_memory() for p in pay]
    a = infer.InferStep(_net(ops, dev, synth, "bf16"), use_graph=True, ingest_size=None, yuv=fmt)
    det = _scenecut().SceneCut(ops, dev, fmt, THRESHOLD)
    A, cuts = {}, []
    for t, p in enumerate(pinned):
        det.push(p)
        is_cut, _, _ = det.pop()
        cuts.append(is_cut)
        a(p, is_new_seq=t == 0 or is_cut)
        if t >= CUT_AT:
            A[t] = _keep(a)
    assert cuts == EXPECT_CUTS and a.n_captures == 1 and a.graph is not None
    b = infer.InferStep(_net(ops, dev, synth, "bf16"), use_graph=True, ingest_size=None, yuv=fmt)
    for t in range(CUT_AT, 9):
        b(pinned[t], is_new_seq=t == CUT_AT)
        for i, (x, y) in enumerate(zip(A[t], _keep(b))):
            assert torch.equal(x, y), (t, i)
        if t == CUT_AT:
            B5 = _keep(b)
    c = infer.InferStep(_net(ops, dev, synth, "bf16"), use_graph=True, ingest_size=None, yuv=fmt)
    for t in range(CUT_AT + 1):
        c(pinned[t], is_new_seq=t == 0)
    C5 = _keep(c)
    assert not torch.equal(C5[1], B5[1]) and not torch.equal(C5[3], B5[3])     # H3 and the denoise payload carry the old scene


# ---------------------------------------------------------------------------------------------------------- 8. the script
def _run(*args, ok=True):
    r = subprocess.run([sys.executable, "predict.py"] + [str(a) for a in args], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r


def _frames_of(path):
    r = _y4m().Y4MReader(str(path), pin=False)
    return [f.numpy().copy() for f in r]


@pytest.mark.gpu
def test_script_scene_cut(tmp_path, synth):
    y = _y4m()
    H, W = 128, 160
    fmt, pay = clip(synth, H, W, "420mpeg2", "LIMITED")
    ref = clip_reference(fmt, pay)
    src = tmp_path / "clip.y4m"
    y.write_file(str(src), y.Header(W, H, "25:1", "p", None, "420mpeg2", "LIMITED"), pay)
    weights = tmp_path / "weights.pt"
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(3).items()}, str(weights))
    common = ("--model_pretrain", weights, "--graph", "1", "--precision", "bf16", "--of_scale", "1", "--y4m_in", src)
    cj, tj = tmp_path / "cuts.json", tmp_path / "timing.json"
    r = _run(*common, "--save", tmp_path / "cut", "--y4m_scene_cut", THRESHOLD, "--y4m_cuts_json", cj, "--timing_json", tj)
    rec = json.load(open(str(cj)))
    assert rec["cuts"] == [CUT_AT] and rec["threshold"] == THRESHOLD
    assert rec["score"] == [v[1] for v in ref] and rec["rel"] == [v[2] for v in ref]
    assert sum("scene cut at frame 5" in line for line in r.stdout.split("\n")) == 1, r.stdout[-2000:]
    timing = json.load(open(str(tj)))
    assert timing["cuts"] == 1 and timing["scene_wait_ms"] >= 0.0 and timing["frames"] == 9
    _run(*common, "--save", tmp_path / "plain", "--timing_json", tmp_path / "t0.json")
    assert "scene_wait_ms" not in json.load(open(str(tmp_path / "t0.json")))
    for kind in ("enhance", "denoise"):
        cut, plain = (_frames_of(tmp_path / d / ("clip_%s.y4m" % kind)) for d in ("cut", "plain"))
        assert len(cut) == 9 and len(plain) == 9, (kind, len(cut), len(plain))
        for t in range(CUT_AT):
            assert np.array_equal(cut[t], plain[t]), (kind, t)
        assert not np.array_equal(cut[CUT_AT], plain[CUT_AT]), kind             # the cache restarted
    r = _run(*common, "--save", tmp_path / "no", "--y4m_cuts_json", tmp_path / "no.json", ok=False)
    assert r.returncode != 0 and "--y4m_cuts_json" in r.stderr and "--y4m_scene_cut" in r.stderr, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "no").exists() and not (tmp_path / "no.json").exists()
