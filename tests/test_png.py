"""Result PNGs encoded on the device (zt_png.hip, `--device_png 1`): round trips through PIL and zlib, the length-limited Huffman
code construction on its own, file size against PIL's writer, determinism, InferStep(png=True), the scripts, and the threaded
writer.  Kernel cases run in the emulator on the CPU and on the MI355X with -m gpu."""
import heapq
import importlib
import io
import json
import os
import struct
import subprocess
import sys
import threading
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import ROOT, frames

PNG_R = 8                                           # scanlines per deflate block (zt_png.hip)


def _utils():
    return importlib.import_module("utils.utils")


def _writer_mod():
    return importlib.import_module("zero-tig_amd.pngwriter")


# ------------------------------------------------------------------------------------------------- helpers
def walk_chunks(data):
    """-> (width, height, concatenated IDAT payload).  Checks the signature, every CRC, the IHDR fields (8-bit, colour type 2,
    deflate, adaptive filtering, no interlace) and that only IHDR, IDAT.., IEND appear, in that order."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, kinds, idat, ihdr = 8, [], [], None
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert len(body) == n and crc == zlib.crc32(tag + body), tag
        kinds.append(tag)
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        pos += 12 + n
    assert pos == len(data)
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and len(kinds) >= 3 and set(kinds[1:-1]) == {b"IDAT"}, kinds
    assert ihdr[2:] == (8, 2, 0, 0, 0), ihdr
    return ihdr[0], ihdr[1], b"".join(idat)


def paeth_scanlines(u8):
    """filter type 4 on every row, as the PNG specification defines it (the encoder's baseline): numpy reference"""
    H, W, _ = u8.shape
    x = u8.reshape(H, 3 * W).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    out = np.empty((H, 3 * W + 1), np.uint8)
    out[:, 0] = 4
    out[:, 1:] = ((x - pred) & 255).astype(np.uint8)
    return out


def check_roundtrip(ops, dev, u8, what):
    data = _utils().png_bytes(torch.from_numpy(u8).to(dev), ops=ops)
    H, W, _ = u8.shape
    w, h, idat = walk_chunks(data)
    assert (w, h) == (W, H), what
    raw = zlib.decompress(idat)                      # verifies the Adler-32
    assert raw == paeth_scanlines(u8).tobytes(), what
    dec = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(dec, u8), what
    return data


def table_frames(synth, H, W):
    """the three frames of the issue's table: quantised low-light frame 3, the same scaled to mean 0.4 ("enhanced"), that plus
    sigma-4 Gaussian noise in 8-bit levels"""
    f = synth.lowlight_frame(3, H, W)[0].transpose(1, 2, 0).astype(np.float64)
    low = np.round(f * 255).astype(np.uint8)
    e = np.clip(f * (0.4 / f.mean()), 0, 1)
    enh = np.clip(e * 255, 0, 255).astype(np.uint8)
    noisy = np.clip(np.round(e * 255 + np.random.default_rng(4).normal(0, 4, e.shape)), 0, 255).astype(np.uint8)
    return {"lowlight": np.ascontiguousarray(low), "enhanced": np.ascontiguousarray(enh), "enhanced_noisy": np.ascontiguousarray(noisy)}


def contents(synth, H, W):
    rng = np.random.default_rng(H * 10007 + W)
    ramp = np.broadcast_to((np.arange(W) * 255 // max(W - 1, 1)).astype(np.uint8)[None, :, None], (H, W, 3))
    out = {"zeros": np.zeros((H, W, 3), np.uint8), "ones": np.full((H, W, 3), 255, np.uint8), "ramp": np.ascontiguousarray(ramp),
           "random": rng.integers(0, 256, (H, W, 3), dtype=np.uint8)}
    out.update(table_frames(synth, H, W))
    return out


# ------------------------------------------------------------------------------------------------- 1. round trip
def test_png_roundtrip(backend, synth):
    """PIL decodes the file to the input pixels, zlib inflates the IDAT payload to the Paeth-filtered scanlines (Adler-32 checked),
    every chunk CRC holds.  Emulator: 1x1, 1x7, 5x33 (one block), 8x16 (exactly one full block), 37x160 (last block of 5 rows);
    MI355X: 1080p and 4K.  Uniform random bytes do not compress: the stream is longer than the raw scanlines."""
    ops, dev, bname = backend
    sizes = [(1, 1), (1, 7), (5, 33), (PNG_R, 16), (37, 160)] if bname == "emu" else [(1080, 1920), (2160, 3840)]
    for H, W in sizes:
        for name, u8 in contents(synth, H, W).items():
            data = check_roundtrip(ops, dev, u8, (H, W, name))
            if name == "random" and H * W >= 5 * 33:
                assert len(walk_chunks(data)[2]) > H * (3 * W + 1), (H, W)
        ws, cap = ops.png_sizes(H, W)
        assert cap >= 2 + 4 + -(-H // PNG_R) * (140 + 15 * (PNG_R * (3 * W + 1) + 1) // 8) and ws > cap


# ------------------------------------------------------------------------------------------------- 2. code lengths
def huffman_cost_and_depth(counts):
    """optimal prefix-code cost (sum of the merged weights; unique) and the depth of one optimal tree (heapq Huffman)"""
    heap = [(int(c), 0) for c in counts if c > 0]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def _histograms(synth):
    fib = np.zeros(257, np.int64)
    a, b = 1, 1
    for s in list(range(23)) + [256]:
        fib[s] = a
        a, b = b, a + b
    two = np.zeros(257, np.int64)
    two[65], two[200] = 1000, 3
    lone = np.zeros(257, np.int64)
    lone[0], lone[256] = PNG_R * (3 * 1920 + 1), 1
    res = np.bincount(paeth_scanlines(table_frames(synth, 64, 1920)["enhanced"]).ravel(), minlength=257).astype(np.int64)
    res[256] = 1
    return {"fibonacci24": fib, "uniform257": np.full(257, 7, np.int64), "two_symbols": two, "literal_and_eob": lone, "residuals": res}


def test_png_code_lengths(backend, synth):
    """Kraft sum exactly 1, at most 15 bits, every occurring symbol coded; optimal cost wherever the unconstrained optimum fits."""
    ops, dev, _ = backend
    hists = _histograms(synth)
    assert huffman_cost_and_depth(hists["fibonacci24"])[1] == 23          # the limiter has to act
    for name, h in hists.items():
        lens = ops.png_code_lengths(torch.from_numpy(h).to(dev)).cpu().numpy().astype(np.int64)
        used = lens > 0
        assert sum(1 << (15 - int(l)) for l in lens[used]) == 1 << 15, (name, lens)
        assert lens.max() <= 15, name
        assert used[h > 0].all(), name
        cost = int((lens * h).sum())
        opt, depth = huffman_cost_and_depth(h)
        print("%s: cost %d bits, unconstrained optimum %d (depth %d)" % (name, cost, opt, depth))
        if depth <= 15:
            assert cost == opt, (name, cost, opt)
        else:
            assert cost >= opt, name


# ------------------------------------------------------------------------------------------------- 3. size against PIL
def test_png_size_against_pil(backend, synth):
    """len(ours) / len(PIL default) on the three table frames at 1080p is at most 1.05 (entropy of the Paeth residuals puts a plain
    Huffman code at 1.005-1.01x, block headers add 0.5 %, Huffman redundancy under 1 %).  Flat content (clean_frame) is printed only:
    without LZ77 matching it compresses worse."""
    ops, dev, _ = backend
    H, W = 1080, 1920
    imgs = table_frames(synth, H, W)
    imgs["clean_frame"] = np.ascontiguousarray(np.clip(synth.clean_frame(3, H, W).transpose(1, 2, 0) * 255, 0, 255).astype(np.uint8))
    ratios = {}
    for name, u8 in imgs.items():
        ours = _utils().png_bytes(torch.from_numpy(u8).to(dev), ops=ops)
        ref = io.BytesIO()
        Image.fromarray(u8).save(ref, "PNG")
        ratios[name] = len(ours) / len(ref.getvalue())
        print("%s: device %d B, PIL %d B, ratio %.4f" % (name, len(ours), len(ref.getvalue()), ratios[name]))
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(ours))), u8)
    for name in ("lowlight", "enhanced", "enhanced_noisy"):
        assert ratios[name] <= 1.05, (name, ratios[name])


# ------------------------------------------------------------------------------------------------- 4. determinism
def test_png_deterministic(backend, synth):
    ops, dev, bname = backend
    H, W = (37, 160) if bname == "emu" else (1080, 1920)
    u8 = torch.from_numpy(table_frames(synth, H, W)["enhanced"]).to(dev)
    a, b = _utils().png_bytes(u8, ops=ops), _utils().png_bytes(u8, ops=ops)
    assert a == b


@pytest.mark.gpu
def test_png_graph_replay_equals_eager(hip_ops, synth):
    """the encode captured into a hipGraph replays to the bytes of the eager launches, also after the input buffer changed"""
    ops, dev = hip_ops
    imgs = table_frames(synth, 540, 960)
    x = torch.from_numpy(imgs["enhanced"]).to(dev)
    eager = {k: _utils().png_bytes(torch.from_numpy(v).to(dev), ops=ops) for k, v in imgs.items()}
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        stream, n = ops.png_encode(x)
    for k in ("lowlight", "enhanced_noisy", "enhanced"):
        x.copy_(torch.from_numpy(imgs[k]))
        g.replay()
        data = stream[:int(n.item())].cpu().numpy()
        assert b"".join(bytes(p) for p in _writer_mod().png_frame(data, 540, 960)) == eager[k], k


# ------------------------------------------------------------------------------------------------- 5. InferStep
@pytest.mark.gpu
def test_inferstep_png(hip_ops, synth):
    """InferStep(png=True) at 540 x 960, bf16: the streams decode to `step.u8` on a new-sequence frame, the eager steady-state
    frame, the captured frame and two replays."""
    ops, dev = hip_ops
    import argparse
    net_mod = importlib.import_module("zero-tig_amd.network")
    net = net_mod.Finetunemodel(argparse.Namespace(dataset="RLV", of_scale=3), ops=ops, precision="bf16")
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(1).items()})
    net = net.to(dev).eval()
    step = importlib.import_module("zero-tig_amd.infer").InferStep(net, use_graph=True, png=True)
    H, W = 540, 960
    for t, x in enumerate(frames(synth, 5, H, W)):
        step(x.pin_memory(), is_new_seq=(t == 0))
        assert (step.graph is not None) == (t >= 2)
        for u8, (stream, n) in zip(step.u8, step.png):
            data = stream[:int(n.item())].cpu().numpy()
            file = b"".join(bytes(p) for p in _writer_mod().png_frame(data, H, W))
            walk_chunks(file)
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(file))), u8.cpu().numpy()), t
    assert step.n_captures == 1


# ------------------------------------------------------------------------------------------------- 6. scripts
def _png_clip(tmp_path, synth, n=4, H=270, W=480):
    data = tmp_path / "data" / "RLV"
    for kind, sub, fn in (("input", "low_light_10", synth.lowlight_frame), ("gt", "normal_light_10", synth.clean_frame)):
        d = data / kind / "S01" / sub
        d.mkdir(parents=True)
        for t in range(n):
            a = np.asarray(fn(t, H, W), dtype=np.float32)
            im = (np.transpose(a[0] if a.ndim == 4 else a, (1, 2, 0)) * 255.0 + 0.5).astype(np.uint8)
            Image.fromarray(im).save(str(d / ("%05d.png" % (t + 1))))
    (data / "train_list.txt").write_text("S01\n")
    (data / "test_list.txt").write_text("S01\n")
    weights = tmp_path / "weights.pt"
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(3).items()}, str(weights))
    return data, weights


def _run(script, *args):
    r = subprocess.run([sys.executable, script] + [str(a) for a in args], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def _png_set(root):
    return {str(p.relative_to(root)): p for p in root.rglob("*.png")}


@pytest.mark.gpu
def test_scripts_device_png(tmp_path, synth):
    """predict.py --graph 1 with --device_png 0 and 1 writes the same file set and every pair of files decodes to identical
    pixels; with --graph 0 the eager encoder writes valid files of the same names; evals.py --device_png 1 writes the Metrics.json
    numbers and the image pixels of --device_png 0."""
    data, weights = _png_clip(tmp_path, synth)
    common = ("--dataset", "RLV", "--lowlight_images_path", data, "--model_pretrain", weights)
    _run("predict.py", *common, "--save", tmp_path / "p0", "--graph", "1", "--device_png", "0")
    _run("predict.py", *common, "--save", tmp_path / "p1", "--graph", "1", "--device_png", "1")
    _run("predict.py", *common, "--save", tmp_path / "p2", "--graph", "0", "--device_png", "1")
    s0, s1, s2 = _png_set(tmp_path / "p0"), _png_set(tmp_path / "p1"), _png_set(tmp_path / "p2")
    assert sorted(s0) == sorted(s1) == sorted(s2) and len(s0) == 8, (sorted(s0), sorted(s1), sorted(s2))
    for nm in s0:
        walk_chunks(s1[nm].read_bytes())
        walk_chunks(s2[nm].read_bytes())
        a, b, c = (np.asarray(Image.open(str(s[nm]))) for s in (s0, s1, s2))
        assert a.shape == (1080, 1920, 3) and np.array_equal(a, b), nm
        assert c.shape == a.shape and c.dtype == a.dtype, nm
    _run("evals.py", *common, "--save", tmp_path / "e0", "--device_png", "0", "--save_images", "2")
    _run("evals.py", *common, "--save", tmp_path / "e1", "--device_png", "1", "--save_images", "2")
    m0, m1 = json.load(open(tmp_path / "e0" / "Metrics.json")), json.load(open(tmp_path / "e1" / "Metrics.json"))
    assert m0 == m1 and m0["images"] == 4, (m0, m1)
    s0, s1 = _png_set(tmp_path / "e0"), _png_set(tmp_path / "e1")
    assert sorted(s0) == sorted(s1) and len(s0) == 6, (sorted(s0), sorted(s1))
    for nm in s0:
        assert np.array_equal(np.asarray(Image.open(str(s0[nm]))), np.asarray(Image.open(str(s1[nm])))), nm


# ------------------------------------------------------------------------------------------------- 7. writer (no kernels)
def _host_stream(u8):
    H, W, _ = u8.shape
    rows = np.zeros((H, 3 * W + 1), np.uint8)               # filter type 0
    rows[:, 1:] = u8.reshape(H, 3 * W)
    return zlib.compress(rows.tobytes(), 1)


def test_writer_files_complete_after_close(tmp_path):
    rng = np.random.default_rng(1)
    imgs = [rng.integers(0, 256, (9 + i, 11, 3), dtype=np.uint8) for i in range(7)]
    w = _writer_mod().PngWriter(slots=2, threads=2)
    for i, u8 in enumerate(imgs):
        stream = _host_stream(u8)
        w.submit_bytes(str(tmp_path / ("%d.png" % i)), stream if i % 2 else np.frombuffer(stream, np.uint8), u8.shape[0], u8.shape[1])
    w.close()
    assert w.files == len(imgs)
    for i, u8 in enumerate(imgs):
        data = (tmp_path / ("%d.png" % i)).read_bytes()
        walk_chunks(data)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), u8)
    big = _writer_mod().png_frame(b"\0" * 2500, 1, 1, idat_bytes=1000)         # several IDAT chunks
    assert [p for p in big if p == b"IDAT"] == [b"IDAT"] * 3 and len(walk_chunks(b"".join(bytes(p) for p in big))[2]) == 2500


def test_writer_bounded_queue_blocks(tmp_path):
    gate, opened = threading.Event(), threading.Event()

    def slow_open(path, mode):
        opened.set()
        assert gate.wait(60)
        return open(path, mode)
    u8 = np.zeros((3, 4, 3), np.uint8)
    w = _writer_mod().PngWriter(slots=2, threads=1, open_fn=slow_open)
    w.submit_bytes(str(tmp_path / "0.png"), _host_stream(u8), 3, 4)
    assert opened.wait(60)                                  # the worker holds job 0; the queue takes two more
    w.submit_bytes(str(tmp_path / "1.png"), _host_stream(u8), 3, 4)
    w.submit_bytes(str(tmp_path / "2.png"), _host_stream(u8), 3, 4)
    t = threading.Thread(target=w.submit_bytes, args=(str(tmp_path / "3.png"), _host_stream(u8), 3, 4), daemon=True)
    t.start()
    t.join(0.5)
    assert t.is_alive(), "a full queue must block the producer"
    gate.set()
    t.join(60)
    assert not t.is_alive()
    w.close()
    assert w.files == 4 and w.wait_writer >= 0.4
    assert sorted(p.name for p in tmp_path.glob("*.png")) == ["0.png", "1.png", "2.png", "3.png"]


def test_writer_failure_surfaces_in_close(tmp_path):
    def bad_open(path, mode):
        raise OSError("disk full: " + path)
    u8 = np.zeros((3, 4, 3), np.uint8)
    w = _writer_mod().PngWriter(slots=2, threads=2, open_fn=bad_open)
    for i in range(5):                                      # later jobs are released, not written: nothing hangs
        try:
            w.submit_bytes(str(tmp_path / ("%d.png" % i)), _host_stream(u8), 3, 4)
        except OSError:
            break
    with pytest.raises(OSError, match="disk full"):
        w.close()
    assert w.files == 0
