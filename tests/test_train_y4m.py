"""Training on raw video (`train.py --y4m_in`): the reader's frame ranges and the rank shares on the host;
`TrainStep(yuv=)` and `InferStep(yuv=, yuv_size=)` against the same steps fed the decoded tensors, bit for bit; the scripts."""
import importlib
import os

import numpy as np
import pytest
import torch

import test_engine as te
import test_y4m as t8
import test_y4m_deep as t16

_y4m = t8._y4m


# ------------------------------------------------------------------------------------------------- 1. host: ranges and shares
def _clip(tmp_path, n=7, W=10, H=6, ctag="420mpeg2"):
    y = _y4m()
    head = y.Header(W, H, "25:1", "p", None, ctag, None)
    rng = np.random.default_rng(9)
    payloads = [rng.integers(0, 256, head.format().frame_bytes, dtype=np.uint8) for _ in range(n)]
    path = tmp_path / "clip.y4m"
    y.write_file(str(path), head, payloads)
    return path, head, payloads


def _read(path, **kw):
    r = _y4m().Y4MReader(str(path) if path is not None else "-", pin=False, **kw)
    return [f.numpy().copy() for f in r]


def test_count_frames_and_rank_shares(tmp_path):
    y = _y4m()
    path, head, payloads = _clip(tmp_path)
    assert y.count_frames(str(path)) == 7
    for world in (1, 2, 3):
        got, steps = [], set()
        for rank in range(world):
            first, count, spe = y.rank_share(7, rank, world)
            steps.add(spe)
            share = _read(path, first=first, count=count)
            assert len(share) == count
            got += share
        # every frame once and in order; every rank makes the same number of steps, the smallest share
        assert len(got) == 7 and all(np.array_equal(a, b) for a, b in zip(got, payloads)), world
        assert steps == {min(y.rank_share(7, r, world)[1] for r in range(world))}
    assert [y.rank_share(7, r, 3) for r in range(3)] == [(0, 3, 1), (3, 3, 1), (6, 1, 1)]
    assert [y.rank_share(7, r, 2) for r in range(2)] == [(0, 4, 3), (4, 3, 3)]
    assert y.rank_share(7, 0, 1) == (0, 7, 7)
    assert [y.rank_share(2, r, 4)[:2] for r in range(4)] == [(0, 1), (1, 1), (2, 0), (3, 0)]      # more ranks than frames


def test_reader_first_count(tmp_path):
    path, head, payloads = _clip(tmp_path)
    for first, count, want in ((0, None, range(7)), (2, 3, range(2, 5)), (5, None, range(5, 7)), (5, 10, range(5, 7)), (3, 0, range(0)),
                               (7, None, range(0)), (9, 2, range(0))):        # `first` at or past the end: an empty iteration
        got = _read(path, first=first, count=count)
        assert len(got) == len(want) and all(np.array_equal(g, payloads[i]) for g, i in zip(got, want)), (first, count)


def test_reader_first_count_on_a_pipe(tmp_path):
    """a pipe cannot seek: the skipped frames are read and dropped, the frames are those of the file"""
    path, head, payloads = _clip(tmp_path)
    y = _y4m()
    for first, count in ((0, None), (2, 3), (6, 5), (8, 1)):
        rd, wr = os.pipe()
        with os.fdopen(wr, "wb") as w:              # 7 small frames fit the pipe's buffer
            w.write(path.read_bytes())
        with os.fdopen(rd, "rb") as fh:
            assert not fh.seekable()
            got = [f.numpy().copy() for f in y.Y4MReader("-", pin=False, fh=fh, first=first, count=count)]
        want = _read(path, first=first, count=count)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), (first, count)


def test_truncated_last_frame_raises(tmp_path):
    y = _y4m()
    path, head, payloads = _clip(tmp_path)
    cut = tmp_path / "cut.y4m"
    cut.write_bytes(path.read_bytes()[:-5])
    with pytest.raises(ValueError, match="truncated"):
        y.count_frames(str(cut))
    with pytest.raises(ValueError, match="truncated"):
        _read(cut, first=4)
    assert len(_read(cut, first=4, count=2)) == 2  # the share ends before the damaged frame
    bad = tmp_path / "bad.y4m"
    bad.write_bytes(path.read_bytes()[:len(head.to_bytes()) + 6 + head.format().frame_bytes] + b"FRAMF\n")
    with pytest.raises(ValueError, match="FRAME"):
        y.count_frames(str(bad))


def test_step_keywords_are_checked_on_the_host():
    y = _y4m()
    optim = importlib.import_module("zero-tig_amd.optim")
    infer = importlib.import_module("zero-tig_amd.infer")
    fmt10 = y.YuvFormat(320, 256, 420, 1, "bt709", 0, 10)
    with pytest.raises(ValueError):
        infer.InferStep(None, ingest_size=(1920, 1080), yuv=fmt10, yuv_size=(160, 128))
    with pytest.raises(ValueError):
        infer.InferStep(None, ingest_size=None, yuv=None, yuv_size=(160, 128))
    step = infer.InferStep(None, ingest_size=None, yuv=fmt10, yuv_size=(160, 128))
    assert step.yuv_format == fmt10.resized(160, 128)
    assert infer.InferStep(None, ingest_size=None, yuv=fmt10, yuv_size=(160, 128), yuv_out_depth=8).yuv_format == \
        fmt10.resized(160, 128)._replace(depth=8)
    with pytest.raises(ValueError):                 # 4:2:0 at an odd size
        infer.InferStep(None, ingest_size=None, yuv=fmt10, yuv_size=(161, 128))
    with pytest.raises(ValueError):
        optim.TrainStep(None, None, yuv=None, yuv_size=(160, 128))
    ts = optim.TrainStep(None, None, yuv=fmt10)
    assert ts.yuv_size == (320, 256) and optim.TrainStep(None, None, yuv=fmt10, yuv_size=(160, 128)).yuv_size == (160, 128)


# ------------------------------------------------------------------------------------------------------------ 2. TrainStep
def _train_run(ops, dev, synth, feed, n=6, **kw):
    """six frames, new sequences at 0 and 4 (test_engine.py's pattern) -> everything a step changes"""
    optim = importlib.import_module("zero-tig_amd.optim")
    net = te._network(ops, dev, synth, 1, of_scale=1).train()
    opt = optim.ClipAdam(net)
    ts = optim.TrainStep(net, opt, **kw)
    ls = [float(ts(feed(t), is_new_seq=(t in (0, 4))).detach()) for t in range(n)]
    bn = net.enhance.conv[1]
    return ts, (ls, opt.fp.flat.clone(), opt.m.clone(), opt.v.clone(), bn.running_mean.clone(), int(bn.num_batches_tracked), net.last_H3.clone())


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for u, v in zip(a[1:], b[1:]):
        assert (u == v) if isinstance(u, int) else torch.equal(u, v)


@pytest.mark.gpu
@pytest.mark.parametrize("ctag", ["420mpeg2", "444p10"])
def test_trainstep_yuv(hip_ops, synth, ctag):
    """TrainStep(yuv=) fed pinned payloads, eager and replayed, == TrainStep fed the decoded tensors: losses of every frame, the
    flat weights, both Adam moments, the BatchNorm running mean and the recurrent cache, bit for bit"""
    ops, dev = hip_ops
    fmt = _y4m().Header(160, 128, None, None, None, ctag, None).format("bt709")
    payloads = [torch.from_numpy(t16._synth_payload(synth, t, fmt).copy()) for t in range(6)]
    _, ref = _train_run(ops, dev, synth, lambda t: ops.yuv_to_planar_f32(payloads[t].to(dev), fmt), use_graph=False)
    for use_graph in (False, True):
        ts, got = _train_run(ops, dev, synth, lambda t: payloads[t].pin_memory(), use_graph=use_graph, yuv=fmt)
        assert (ts.graph is not None) == use_graph and (not use_graph or tuple(ts.x.shape) == (1, 3, 128, 160))
        assert ts.loaded is not None and ts.loaded.query()
        _same(ref, got)


@pytest.mark.gpu
def test_trainstep_yuv_sized(hip_ops, synth):
    """the same with yuv_size: a 256 x 320 C420p10 stream trained at 128 x 160 == a TrainStep fed `yuv_to_planar_f32_sized` tensors"""
    ops, dev = hip_ops
    fmt = _y4m().Header(320, 256, None, None, None, "420p10", None).format("bt709")
    payloads = [torch.from_numpy(t16._synth_payload(synth, t, fmt).copy()) for t in range(6)]
    _, ref = _train_run(ops, dev, synth, lambda t: ops.yuv_to_planar_f32_sized(payloads[t].to(dev), fmt, (160, 128)), use_graph=False)
    ts, got = _train_run(ops, dev, synth, lambda t: payloads[t].pin_memory(), use_graph=True, yuv=fmt, yuv_size=(160, 128))
    assert ts.graph is not None and tuple(ts.x.shape) == (1, 3, 128, 160)
    _same(ref, got)


# ------------------------------------------------------------------------------------------------------------ 3. InferStep
@pytest.mark.gpu
def test_inferstep_yuv_sized(hip_ops, synth):
    """five frames of a 256 x 320 C420p10 stream through InferStep(yuv=, yuv_size=(160, 128)), replayed and eager, == an InferStep
    without yuv fed the sized tensor; the payloads are the encode of H2 / H3 at the reduced size; one capture"""
    ops, dev = hip_ops
    infer = importlib.import_module("zero-tig_amd.infer")
    fmt10 = _y4m().Header(320, 256, None, None, None, "420p10", None).format("bt709")
    out_fmt = fmt10.resized(160, 128)
    payloads = [torch.from_numpy(t16._synth_payload(synth, t, fmt10).copy()) for t in range(5)]
    sized = [ops.yuv_to_planar_f32_sized(p.to(dev), fmt10, (160, 128)) for p in payloads]
    for use_graph in (True, False):
        step = infer.InferStep(t8._net(ops, dev, synth, "bf16"), use_graph=use_graph, ingest_size=None, yuv=fmt10, yuv_size=(160, 128))
        ref = infer.InferStep(t8._net(ops, dev, synth, "bf16"), use_graph=use_graph, ingest_size=None)
        assert step.yuv_format == out_fmt
        for t in range(5):
            H2, H3, _ = step(payloads[t].pin_memory(), is_new_seq=t == 0)
            R2, R3, _ = ref(sized[t], is_new_seq=t == 0)
            assert torch.equal(H2, R2) and torch.equal(H3, R3), (use_graph, t)
            if use_graph:
                assert torch.equal(step.x, sized[t]), t
            for i, Hx in enumerate((H2, H3)):
                assert step.yuv[i].numel() == out_fmt.frame_bytes
                assert torch.equal(step.yuv[i], ops.rgb_f32_to_yuv(Hx, out_fmt)), (use_graph, t, i)
        assert step.n_captures == (1 if use_graph else 0)
    with pytest.raises(ValueError):
        infer.InferStep(None, ingest_size=(1920, 1080), yuv=fmt10, yuv_size=(160, 128))


# ------------------------------------------------------------------------------------------------------------ 4. the scripts
def _train_dir(save):
    return [d for d in save.iterdir() if d.name.startswith("Train-")][0]


@pytest.mark.gpu
def test_scripts_train_y4m(tmp_path, synth):
    y = _y4m()
    n, H, W = 6, 128, 160
    head = y.Header(W, H, "30000:1001", "p", None, "420p10", "LIMITED")
    fmt = head.format("bt709")
    src = tmp_path / "clip.y4m"
    y.write_file(str(src), head, [t16._synth_payload(synth, t, fmt) for t in range(n)])
    common = ("--y4m_in", src, "--of_scale", "1", "--epochs", "2", "--seed", "5")
    r = t8._run("train.py", *common, "--save", tmp_path / "a")
    tr = _train_dir(tmp_path / "a")
    for f in ("model_epochs/weights_0.pt", "model_epochs/weights_1.pt", "model_epochs/resume.pt", "log.txt"):
        assert (tr / f).exists(), f
    ck = torch.load(str(tr / "model_epochs" / "resume.pt"))
    assert ck["epoch"] == 2 and ck["step"] == 12
    for epoch in (0, 1):
        for kind in ("enhance", "denoise"):
            h, frames = t8._frames_of(tr / "result" / ("clip_%s_%d.y4m" % (kind, epoch)))
            assert h == head and len(frames) == n and all(f.size == fmt.frame_bytes for f in frames), (kind, epoch, h, len(frames))
    assert "train-epoch 001" in r.stdout and "train-epoch 001 005 " in r.stdout and "train-epoch 001 006 " not in r.stdout
    lines = [l for l in r.stdout.splitlines() if "throughput" in l]
    assert len(lines) == 2 and all("y4m -> PCIe (payload) -> device decode -> step" in l for l in lines), lines
    # the same seed gives the same weights byte for byte; --y4m_preview 2 writes two frames per stream
    t8._run("train.py", *common, "--save", tmp_path / "b", "--y4m_preview", "2")
    tr2 = _train_dir(tmp_path / "b")
    assert (tr2 / "model_epochs" / "weights_1.pt").read_bytes() == (tr / "model_epochs" / "weights_1.pt").read_bytes()
    for kind in ("enhance", "denoise"):
        h, frames = t8._frames_of(tr2 / "result" / ("clip_%s_1.y4m" % kind))
        assert h == head and len(frames) == 2
    # refusals
    r = t8._run("train.py", "--y4m_in", "-", "--epochs", "2", "--save", tmp_path / "no", ok=False)
    assert r.returncode == 2 and "--y4m_in -" in r.stderr and "--epochs" in r.stderr, (r.returncode, r.stderr[-500:])
    r = t8._run("train.py", "--y4m_size", "96x64", "--save", tmp_path / "no", ok=False)
    assert r.returncode == 2 and "--y4m_size" in r.stderr and "--y4m_in" in r.stderr, (r.returncode, r.stderr[-500:])
    r = t8._run("train.py", "--y4m_in", src, "--host_ingest", "--save", tmp_path / "no", ok=False)
    assert r.returncode == 2 and "--y4m_in" in r.stderr and "--host_ingest" in r.stderr, (r.returncode, r.stderr[-500:])
    assert not (tmp_path / "no").exists()
    # the trained weights, at another size.  144 x 136 and not a smaller one: RAFT's four-level correlation pyramid needs
    # H / 8 >= 16 and W / 8 >= 16 at of_scale 1 (zt_corr_lookup rejects a 1-pixel level), so 128 pixels is the least a steady-state
    # frame can have; the width shrinks (160 -> 144) and the height grows (128 -> 136), so both passes of the resize run
    weights = tr / "model_epochs" / "weights_1.pt"
    pred = ("predict.py", "--graph", "1", "--of_scale", "1", "--y4m_in", src, "--y4m_size", "144x136", "--model_pretrain", weights)
    t8._run(*pred, "--save", tmp_path / "pred")
    for kind in ("enhance", "denoise"):
        h, frames = t8._frames_of(tmp_path / "pred" / ("clip_%s.y4m" % kind))
        assert h == head.resized(144, 136) and len(frames) == n and all(f.size == fmt.resized(144, 136).frame_bytes for f in frames), (kind, h)
    r = t8._run(*pred, "--save", tmp_path / "no", "--y4m_resize", "1", ok=False)
    assert r.returncode == 2 and "--y4m_size" in r.stderr and "--y4m_resize" in r.stderr, (r.returncode, r.stderr[-500:])
