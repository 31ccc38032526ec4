"""Mode 2 of the device PNG encoder (zt_png.hip, `--device_png 2`): per block of 8 rows a second tokenisation with run-length
matches (length 3..258, distance 1), chosen where it is strictly shorter.  Round trips through PIL and zlib, the exact token
sequence of every block that uses matches against a reference tokeniser, the run / thread / packing-chunk / block boundaries,
stream size against mode 1 and against zlib's Z_RLE, determinism, graph replay, InferStep(png=2) and the scripts.  Kernel cases
run in the emulator on the CPU and on the MI355X with -m gpu."""
import importlib
import io
import json
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from test_png import PNG_R, _png_clip, _png_set, _run, _utils, _writer_mod, contents, paeth_scanlines, table_frames, walk_chunks

MAXMATCH = 258


# ------------------------------------------------------------------------------------------------- helpers
def unfilter_paeth(scanlines):
    """inverse of `paeth_scanlines`: uint8 [H][1 + 3 W] scanlines, filter type 4 on every row -> uint8 [H][W][3], so that a
    test dictates the exact residual bytes the encoder sees"""
    sc = np.asarray(scanlines, np.uint8)
    H, rb = sc.shape
    assert (rb - 1) % 3 == 0 and (sc[:, 0] == 4).all()
    n = rb - 1
    prev = [0] * n
    rows = []
    for y in range(H):
        res, cur = sc[y, 1:].tolist(), [0] * n
        for x in range(n):
            a = cur[x - 3] if x >= 3 else 0
            b = prev[x]
            c = prev[x - 3] if x >= 3 else 0
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            cur[x] = (res[x] + (a if pa <= pb and pa <= pc else (b if pb <= pc else c))) & 255
        rows.append(cur)
        prev = cur
    return np.ascontiguousarray(np.array(rows, np.uint8).reshape(H, n // 3, 3))


class _Bits:
    def __init__(self, data):
        self.data, self.pos, self.buf, self.n = data, 0, 0, 0

    def need(self, k):
        while self.n < k:
            self.buf |= (self.data[self.pos] if self.pos < len(self.data) else 0) << self.n
            self.pos += 1
            self.n += 8

    def take(self, k):
        self.need(k)
        v = self.buf & ((1 << k) - 1)
        self.buf >>= k
        self.n -= k
        return v

    def bitpos(self):
        return 8 * self.pos - self.n

    def align(self):
        self.take(self.n & 7)


def _decoder(lengths):
    """canonical code lengths -> (lookup over max-length bits read LSB first -> (symbol, length), max length)"""
    mx = max(lengths)
    count = [0] * (mx + 2)
    for l in lengths:
        count[l] += l > 0
    code, nxt = 0, [0] * (mx + 2)
    for l in range(1, mx + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = [None] * (1 << mx)
    for s, l in enumerate(lengths):
        if l:
            c, nxt[l] = nxt[l], nxt[l] + 1
            rev = int(format(c, "0%db" % l)[::-1], 2)
            for hi in range(1 << (mx - l)):
                table[rev | (hi << l)] = (s, l)
    return table, mx


def _symbol(bits, dec):
    table, mx = dec
    bits.need(mx)
    s, l = table[bits.buf & ((1 << mx) - 1)]
    bits.take(l)
    return s


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
          16385, 24577]
_DEXT = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
_CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def deflate_blocks(stream):
    """zlib stream -> list of blocks: {"btype", "hlit", "hdist", "tokens", "bit0", "bit1"} with tokens = byte values and
    (length, distance) pairs, bit positions counted from the first block.  A small pure-Python inflate (RFC 1951), no fixed codes."""
    assert stream[0] == 0x78 and (stream[0] * 256 + stream[1]) % 31 == 0
    bits, blocks = _Bits(stream[2:]), []
    while True:
        blk = {"bit0": bits.bitpos()}
        final, btype = bits.take(1), bits.take(2)
        blk["btype"] = btype
        if btype == 0:
            bits.align()
            ln, nln = bits.take(16), bits.take(16)
            assert ln ^ nln == 0xFFFF
            blk.update(hlit=None, hdist=None, tokens=[bits.take(8) for _ in range(ln)])
        else:
            assert btype == 2, btype
            hlit, hdist, hclen = bits.take(5), bits.take(5), bits.take(4)
            cl = [0] * 19
            for i in range(hclen + 4):
                cl[_CLORDER[i]] = bits.take(3)
            cdec, lens = _decoder(cl), []
            while len(lens) < hlit + 257 + hdist + 1:
                s = _symbol(bits, cdec)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + bits.take(2))
                else:
                    lens += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
            assert len(lens) == hlit + 257 + hdist + 1
            ldec = _decoder(lens[:hlit + 257])
            dl = lens[hlit + 257:]
            ddec = _decoder(dl) if any(dl) else None
            tokens = []
            while True:
                s = _symbol(bits, ldec)
                if s < 256:
                    tokens.append(s)
                elif s == 256:
                    break
                else:
                    ln = _LBASE[s - 257] + bits.take(_LEXT[s - 257])
                    d = _symbol(bits, ddec)
                    tokens.append((ln, _DBASE[d] + bits.take(_DEXT[d])))
            blk.update(hlit=hlit, hdist=hdist, tokens=tokens, dist_lengths=dl)
        blk["bit1"] = bits.bitpos()
        blocks.append(blk)
        if final:
            return blocks


def rle_tokens(block):
    """the run tokenisation of one block's filtered bytes: first byte of a run a literal, the rest cut from the run's start into
    chunks of 258; 3..258 -> (length, 1), a final chunk of 1 or 2 -> literals"""
    b = np.asarray(block, np.uint8)
    cuts = np.flatnonzero(np.diff(b.astype(np.int16)) != 0) + 1
    out = []
    for s, e in zip(np.concatenate([[0], cuts]).tolist(), np.concatenate([cuts, [len(b)]]).tolist()):
        v, m = int(b[s]), e - s - 1
        out.append(v)
        while m > 0:
            c = min(m, MAXMATCH)
            out += [(c, 1)] if c >= 3 else [v] * c
            m -= c
    return out


def encode(ops, dev, u8, mode):
    return _utils().png_bytes(torch.from_numpy(u8).to(dev), ops=ops, mode=mode)


def check_case(ops, dev, u8, what, tokens=True, expect_matches=None):
    """round trip of the mode-2 file, never longer than mode 1; with `tokens`, every deflate block against the token rules and the
    mode-1 block.  -> (mode-1 file, mode-2 file, blocks of the mode-2 stream or None)"""
    H, W, _ = u8.shape
    one, two = encode(ops, dev, u8, 1), encode(ops, dev, u8, 2)
    w, h, idat = walk_chunks(two)
    assert (w, h) == (W, H), what
    sc = paeth_scanlines(u8)
    assert zlib.decompress(idat) == sc.tobytes(), what                  # verifies the Adler-32
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(two)).convert("RGB")), u8), what
    assert len(two) <= len(one), (what, len(two), len(one))
    if not tokens:
        return one, two, None
    idat1 = walk_chunks(one)[2]
    b1, b2 = deflate_blocks(idat1), deflate_blocks(idat)
    nblk = -(-H // PNG_R)
    assert len(b1) == len(b2) == 2 * nblk - 1, what
    any_match = False
    for k in range(nblk):
        x1, x2 = b1[2 * k], b2[2 * k]
        raw = sc[k * PNG_R:(k + 1) * PNG_R].ravel()
        toks = x2["tokens"]
        assert x2["btype"] == 2 and x2["hdist"] == 0 and x1["hlit"] == 0, (what, k)
        assert x2["bit0"] % 8 == 0 and isinstance(toks[0], int), (what, k)   # no match reaches into the previous block
        matches = [t for t in toks if not isinstance(t, int)]
        assert all(d == 1 and 3 <= ln <= MAXMATCH for ln, d in matches), (what, k)
        assert x2["bit1"] - x2["bit0"] <= x1["bit1"] - x1["bit0"], (what, k)
        if matches:
            any_match = True
            assert x2["bit1"] - x2["bit0"] < x1["bit1"] - x1["bit0"], (what, k)     # chosen only where strictly shorter
            assert x2["dist_lengths"] == [1], (what, k)
            assert toks == rle_tokens(raw), (what, k)
        else:                                                                        # written exactly as mode 1 writes it
            assert x2["hlit"] == 0 and toks == raw.tolist(), (what, k)
            assert idat[2 + x2["bit0"] // 8:2 + -(-x2["bit1"] // 8)] == idat1[2 + x1["bit0"] // 8:2 + -(-x1["bit1"] // 8)], (what, k)
        if k < nblk - 1:
            assert b2[2 * k + 1]["btype"] == 0 and b2[2 * k + 1]["tokens"] == [], (what, k)
    if expect_matches is not None:
        assert any_match == expect_matches, what
    return one, two, b2


def _filler(n, rng, avoid):
    """n bytes without two equal neighbours and without the values in `avoid`"""
    vals = np.array([v for v in range(256) if v not in avoid], np.uint8)
    idx = rng.integers(0, len(vals), n)
    idx[1:] = np.where(idx[1:] == idx[:-1], (idx[1:] + 1) % len(vals), idx[1:])
    for i in range(1, n):                                   # the fix-up above can collide with the next one
        if idx[i] == idx[i - 1]:
            idx[i] = (idx[i] + 1) % len(vals)
    return vals[idx]


RUNS = [1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 517, 518, 519]


def _crafted_rows(W, runs, va, vb, rng):
    """scanlines whose rows hold the runs one after the other in alternating values va / vb (a run that does not fit starts the
    next row), the rest of each row filled without repeats"""
    rb = 1 + 3 * W
    rows, cur, flip = [], [4], 0
    for L in runs:
        assert L < rb
        if len(cur) + L > rb:
            rows.append(cur)
            cur = [4]
        cur += [vb if flip else va] * L
        flip ^= 1
    rows.append(cur)
    out = np.empty((len(rows), rb), np.uint8)
    for y, r in enumerate(rows):
        out[y, :len(r)] = r
        out[y, len(r):] = _filler(rb - len(r), rng, {4, va, vb})
    return out


# ------------------------------------------------------------------------------------------------- 1. round trip and tokens
def test_rle_crafted_runs(backend):
    """run lengths at the edges of the scheme (smallest match; remainders 0 / 1 / 2 / 3 after the first literal and one or two full
    chunks), in alternating values: as 1 x 300 images (one per row of runs) and all of them in one 8 x 300 image"""
    ops, dev, _ = backend
    rng = np.random.default_rng(11)
    for va, vb in ((0, 255), (7, 8)):
        sc = _crafted_rows(300, RUNS, va, vb, rng)
        assert sc.shape[0] <= PNG_R
        for y in range(sc.shape[0]):
            _, _, blocks = check_case(ops, dev, unfilter_paeth(sc[y:y + 1]), ("row", y, va, vb), expect_matches=True)
            assert blocks[0]["tokens"] == rle_tokens(sc[y])
        full = np.concatenate([sc] + [np.concatenate([[4], _filler(900, rng, {4})])[None].astype(np.uint8)
                                      for _ in range(PNG_R - sc.shape[0])])
        _, _, blocks = check_case(ops, dev, unfilter_paeth(full), ("8x300", va, vb), expect_matches=True)
        lens = [t[0] for t in blocks[0]["tokens"] if not isinstance(t, int)]
        want = []
        for L in RUNS:
            m = L - 1
            want += [MAXMATCH] * (m // MAXMATCH) + ([m % MAXMATCH] if m % MAXMATCH >= 3 else [])
        assert lens == want, (lens, want)


def test_rle_filter_byte_joins_run(backend):
    """residual all 4 on 9 x 87: the filter byte 4 of every row joins the run; block 0 is one run of 8 * 262 bytes, the last block
    has one row"""
    ops, dev, _ = backend
    sc = np.full((9, 262), 4, np.uint8)
    _, _, blocks = check_case(ops, dev, unfilter_paeth(sc), "all4", expect_matches=True)
    assert blocks[0]["tokens"] == [4] + [(MAXMATCH, 1)] * 8 + [(8 * 262 - 1 - 8 * MAXMATCH, 1)]
    assert blocks[2]["tokens"] == [4, (MAXMATCH, 1), (3, 1)]


def _with_runs(H, W, runs, rng):
    """random scanlines with runs (first position, last position, value) over the flattened block; a run may cross a row start
    only with value 4"""
    rb = 1 + 3 * W
    sc = rng.integers(0, 256, (H, rb), dtype=np.uint8)
    flat = sc.reshape(-1)
    for a, b, v in runs:
        flat[a:b + 1] = v
        assert v == 4 or a // rb == b // rb and a % rb > 0, (a, b, v)
    sc[:, 0] = 4
    return sc


def test_rle_thread_and_chunk_boundaries(backend):
    """runs that end exactly at, and runs that straddle, the per-thread boundary (32 positions) and the packing-chunk boundary
    (8192 positions; 8 x 2731 has rows of 8194 bytes); a run up to the last byte of the block; one run over nine packing chunks.
    Every image also has one long run elsewhere, so that the block is written with matches whatever the run under test saves."""
    ops, dev, _ = backend
    rng = np.random.default_rng(12)
    n37 = 5 * 481                                                        # last block of 37 x 160
    small = [[(20, 31, 9)], [(28, 36, 9)], [(29, 31, 9), (32, 34, 10)], [(1, 64, 9)], [(33, 63, 9), (64, 95, 10)],
             [(481 - 100, 481 + 100, 4)], [(8 * 481 - 5, 8 * 481 - 1, 9)]]
    for runs in small:
        check_case(ops, dev, unfilter_paeth(_with_runs(8, 160, runs + [(2000, 2400, 77)], rng)), ("8x160", runs), expect_matches=True)
    sc = _with_runs(37, 160, [(32 * 481 + n37 - 40, 32 * 481 + n37 - 1, 9)], rng)
    _, _, blocks = check_case(ops, dev, unfilter_paeth(sc), "37x160 tail", expect_matches=True)
    assert blocks[-1]["tokens"][-1] == (39, 1)                           # the run ends at n - 1
    rb, n = 8194, 8 * 8194
    big = [[(8000, 8191, 9)], [(8000, 8193, 9)], [(8192, 8193, 9)], [(8000, 8300, 4)], [(7933, 8192, 9)],
           [(8190, 8193, 9)], [(16383 - 258, 16383, 9), (16384, 16387, 10)], [(n - 300, n - 1, 9)]]
    for runs in big:
        sc = _with_runs(8, 2731, runs + [(30000, 30600, 77)], rng)
        _, _, blocks = check_case(ops, dev, unfilter_paeth(sc), ("8x2731", runs), expect_matches=True)
    assert blocks[0]["tokens"][-2:] == [(MAXMATCH, 1), (41, 1)]
    _, two, blocks = check_case(ops, dev, unfilter_paeth(np.full((8, rb), 4, np.uint8)), "8x2731 all 4", expect_matches=True)
    assert blocks[0]["tokens"] == [4] + [(MAXMATCH, 1)] * ((n - 1) // MAXMATCH) + [((n - 1) % MAXMATCH, 1)]
    # blocks of exactly one and two packing chunks (8 x 341: n = 8192; 4 x 1365: n = 16384): the end-of-block symbol is alone in a
    # chunk of its own
    for H, W in ((8, 341), (4, 1365)):
        rb, n = 1 + 3 * W, H * (1 + 3 * W)
        assert n % 8192 == 0
        check_case(ops, dev, np.zeros((H, W, 3), np.uint8), (H, W, "zeros"), expect_matches=True)
        _, _, blocks = check_case(ops, dev, unfilter_paeth(np.full((H, rb), 4, np.uint8)), (H, W, "all 4"), expect_matches=True)
        assert blocks[0]["tokens"] == [4] + [(MAXMATCH, 1)] * ((n - 1) // MAXMATCH) + [((n - 1) % MAXMATCH, 1)]
        # a run up to n - 1; one whose 259th byte is a thread's first position; a smallest match at the very end
        for runs in ([(n - 300, n - 1, 9)], [(n - rb + 320 - 259, n - rb + 400, 9)], [(n - 4, n - 1, 9)]):
            sc = _with_runs(H, W, runs + [(rb + 100, rb + 700, 77)], rng)
            _, _, blocks = check_case(ops, dev, unfilter_paeth(sc), (H, W, runs), expect_matches=True)
        assert blocks[0]["tokens"][-1] == (3, 1)


def test_rle_run_across_blocks(backend):
    """a constant 17 x 160 image: the run is cut at every 8-row block, each block starts with a literal"""
    ops, dev, _ = backend
    for v in (0, 200):
        _, _, blocks = check_case(ops, dev, np.full((17, 160, 3), v, np.uint8), ("const", v), expect_matches=True)
        assert [len(b["tokens"]) > 0 for b in blocks] == [True, False, True, False, True]


def test_rle_contents(backend, synth):
    """the frames of test_png.py: emulator 1x1, 1x2, 5x33, 8x16, 37x160; MI355X 37x160, 8x2731 and 17x3840 (a block of 92 KB, larger
    than any staging).  Uniform random bytes have no run worth a match: the bytes of mode 1."""
    ops, dev, bname = backend
    sizes = [(1, 1), (1, 2), (5, 33), (PNG_R, 16), (37, 160)] if bname == "emu" else [(37, 160), (PNG_R, 2731), (17, 3840)]
    for H, W in sizes:
        for name, u8 in contents(synth, H, W).items():
            one, two, _ = check_case(ops, dev, u8, (H, W, name), tokens=H * W <= PNG_R * 2731)
            if name == "random":
                assert two == one, (H, W)
            if name in ("zeros", "ones") and H * W >= 5 * 33:
                assert len(two) < len(one), (H, W, name)


# ------------------------------------------------------------------------------------------------- 2. size
def _stream_len(data):
    return len(walk_chunks(data)[2])


def _zlib_rle_len(u8):
    """zlib Z_RLE on the same Paeth scanlines, one raw deflate stream per 8 rows (level 6) + 5 bytes each, + 6"""
    sc, total = paeth_scanlines(u8), 6
    for y in range(0, sc.shape[0], PNG_R):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        total += len(c.compress(sc[y:y + PNG_R].tobytes()) + c.flush()) + 5
    return total


def test_rle_size(backend, synth):
    """1080p zlib streams.  zeros: mode 2 at most 1/20 of mode 1 (cost model of the stream: 1/27).  enhanced_noisy with rows 0-137
    and 942-1079 black ("letterbox") and with its left half black: at most 1.01 x zlib Z_RLE per 8 rows (model 1.0011 / 1.0013) and
    at most 0.97 x / 0.85 x mode 1 (model 0.957 / 0.806).  The table frames and clean_frame: never longer than mode 1."""
    ops, dev, _ = backend
    H, W = 1080, 1920
    imgs = table_frames(synth, H, W)
    imgs["clean_frame"] = np.ascontiguousarray(np.clip(synth.clean_frame(3, H, W).transpose(1, 2, 0) * 255, 0, 255).astype(np.uint8))
    letterbox, half = imgs["enhanced_noisy"].copy(), imgs["enhanced_noisy"].copy()
    letterbox[:138] = 0
    letterbox[942:] = 0
    half[:, :W // 2] = 0
    cases = dict(imgs, zeros=np.zeros((H, W, 3), np.uint8), letterbox=letterbox, half_black=half)
    fig = {}
    for name, u8 in cases.items():
        one, two = encode(ops, dev, u8, 1), encode(ops, dev, u8, 2)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(two))), u8), name
        fig[name] = (_stream_len(one), _stream_len(two), one == two)
        print("%s: mode 1 %d B, mode 2 %d B, ratio %.4f, identical bytes: %s" % (name, fig[name][0], fig[name][1],
                                                                               fig[name][1] / fig[name][0], one == two))
    ref = {name: _zlib_rle_len(cases[name]) for name in ("letterbox", "half_black", "zeros")}
    for name, r in ref.items():
        print("%s: zlib Z_RLE per 8 rows %d B, mode 2 / Z_RLE %.4f" % (name, r, fig[name][1] / r))
    assert fig["zeros"][1] * 20 <= fig["zeros"][0], fig["zeros"]
    for name, bound in (("letterbox", 0.97), ("half_black", 0.85)):
        assert fig[name][1] <= 1.01 * ref[name], (name, fig[name], ref[name])
        assert fig[name][1] <= bound * fig[name][0], (name, fig[name])
    for name in ("lowlight", "enhanced", "enhanced_noisy", "clean_frame"):
        assert fig[name][1] <= fig[name][0], (name, fig[name])


# ------------------------------------------------------------------------------------------------- 3. determinism
def test_rle_deterministic(backend, synth):
    ops, dev, _ = backend
    u8 = table_frames(synth, 37, 160)["enhanced"].copy()
    u8[:, :80] = 0
    a, b = encode(ops, dev, u8, 2), encode(ops, dev, u8, 2)
    assert a == b and a != encode(ops, dev, u8, 1)


def test_rle_mode_argument(backend):
    ops, dev, _ = backend
    u8 = torch.zeros((3, 5, 3), dtype=torch.uint8, device=dev)
    ws_bytes, cap = ops.png_sizes(3, 5)
    ws, out = torch.empty(ws_bytes, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev)
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    for mode in (0, 3, -1):
        with pytest.raises(RuntimeError, match="invalid argument"):
            ops.lib.call("zt_png_encode_u8_mode", u8, 3, 5, mode, ws, ws_bytes, out, cap, n, None)
    streams = []
    for name, args in (("zt_png_encode_u8", ()), ("zt_png_encode_u8_mode", (1,))):      # the old entry point means mode 1
        ops.lib.call(name, u8, 3, 5, *args, ws, ws_bytes, out, cap, n, ops._s(u8))
        streams.append(bytes(out[:int(n.item())].cpu().numpy()))
    assert streams[0] == streams[1]


# ------------------------------------------------------------------------------------------------- 4. MI355X only
@pytest.mark.gpu
def test_rle_graph_replay_equals_eager(hip_ops, synth):
    """mode 2 captured into a hipGraph replays to the bytes of the eager launches, also after the input buffer changed"""
    ops, dev = hip_ops
    for H, W in ((37, 160), (17, 3840)):
        imgs = contents(synth, H, W)
        imgs["half"] = imgs["enhanced_noisy"].copy()
        imgs["half"][:, :W // 2] = 0
        eager = {k: encode(ops, dev, v, 2) for k, v in imgs.items()}
        x = torch.from_numpy(imgs["enhanced"]).to(dev)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            stream, n = ops.png_encode(x, mode=2)
        for k in ("zeros", "half", "random", "enhanced"):
            x.copy_(torch.from_numpy(imgs[k]))
            g.replay()
            data = stream[:int(n.item())].cpu().numpy()
            assert b"".join(bytes(p) for p in _writer_mod().png_frame(data, H, W)) == eager[k], (H, W, k)


def _file(stream_n, H, W):
    stream, n = stream_n
    return b"".join(bytes(p) for p in _writer_mod().png_frame(stream[:int(n.item())].cpu().numpy(), H, W))


@pytest.mark.gpu
def test_inferstep_png_mode2(hip_ops, synth):
    """InferStep(png=2) on a 4-frame 270 x 480 clip of decoded uint8 frames (ingested to 1080p as predict.py does), bf16: the
    streams decode to `step.u8` and are the mode-2 bytes of `step.u8` on the new-sequence, the eager, the captured and the replayed
    frame; InferStep(png=True) on the same clip still gives the mode-1 bytes"""
    ops, dev = hip_ops
    import argparse
    net_mod = importlib.import_module("zero-tig_amd.network")
    clip = [torch.from_numpy(np.ascontiguousarray((np.transpose(synth.lowlight_frame(t, 270, 480)[0], (1, 2, 0)) * 255.0 + 0.5)
                                                  .astype(np.uint8))) for t in range(4)]
    H, W = 1080, 1920
    for png, mode in ((2, 2), (True, 1)):
        net = net_mod.Finetunemodel(argparse.Namespace(dataset="RLV", of_scale=3), ops=ops, precision="bf16")
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_state(1).items()})
        net = net.to(dev).eval()
        step = importlib.import_module("zero-tig_amd.infer").InferStep(net, use_graph=True, png=png)
        for t, x in enumerate(clip):
            step(x.pin_memory(), is_new_seq=(t == 0))
            assert (step.graph is not None) == (t >= 2)
            for u8, sn in zip(step.u8, step.png):
                assert tuple(u8.shape) == (H, W, 3)
                file = _file(sn, H, W)
                walk_chunks(file)
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(file))), u8.cpu().numpy()), (png, t)
                assert file == _utils().png_bytes(u8.clone(), ops=ops, mode=mode), (png, t)
        assert step.n_captures == 1


@pytest.mark.gpu
def test_scripts_device_png_mode2(tmp_path, synth):
    """predict.py --device_png 2 writes the file set of --device_png 0 and every file decodes to its pixels, with --graph 1 and with
    --graph 0 (each against the --device_png 0 run of the same --graph: the eager forward and the streaming plan may differ by a
    level); evals.py --device_png 2 --save_images 4 writes the twelve files of --device_png 0 with the same pixels and the same
    Metrics.json.  Each script in a fresh child process."""
    data, weights = _png_clip(tmp_path, synth)
    common = ("--dataset", "RLV", "--lowlight_images_path", data, "--model_pretrain", weights)
    for graph in ("1", "0"):
        ref, out = tmp_path / ("p0_g" + graph), tmp_path / ("p2_g" + graph)
        _run("predict.py", *common, "--save", ref, "--graph", graph, "--device_png", "0")
        _run("predict.py", *common, "--save", out, "--graph", graph, "--device_png", "2")
        s0, s2 = _png_set(ref), _png_set(out)
        assert sorted(s0) == sorted(s2) and len(s0) == 8, (graph, sorted(s0), sorted(s2))
        for nm in s0:
            walk_chunks(s2[nm].read_bytes())
            a, b = np.asarray(Image.open(str(s0[nm]))), np.asarray(Image.open(str(s2[nm])))
            assert a.shape == (1080, 1920, 3) and b.dtype == a.dtype and np.array_equal(a, b), (graph, nm)
    _run("evals.py", *common, "--save", tmp_path / "e0", "--device_png", "0", "--save_images", "4")
    _run("evals.py", *common, "--save", tmp_path / "e2", "--device_png", "2", "--save_images", "4")
    m0, m2 = json.load(open(tmp_path / "e0" / "Metrics.json")), json.load(open(tmp_path / "e2" / "Metrics.json"))
    assert m0 == m2 and m2["images"] == 4, (m0, m2)
    s0, s2 = _png_set(tmp_path / "e0"), _png_set(tmp_path / "e2")
    assert sorted(s0) == sorted(s2) and len(s2) == 12, (sorted(s0), sorted(s2))
    for nm in s2:
        w, h, _ = walk_chunks(s2[nm].read_bytes())
        a, b = np.asarray(Image.open(str(s0[nm]))), np.asarray(Image.open(str(s2[nm])))
        assert b.shape == (h, w, 3) and np.array_equal(a, b), nm
