"""The grading of evals.py's video mode: the metric table the kernels write into, and one grader per family of
metrics.  A grader registers its columns with the table, and then
  launch(ctx, ri, rf)    queues the frame's kernels, which write into its columns of the device row (ri, rf); never synchronises
  read(n, rec, ri, rf)   host only, one chunk later: the same row as lists -> totals, the frame's record `rec`, the log lines of
                         frame n (counted from 1)
  summary(result)        its keys of Metrics.json (result["images"] is the frame count) and its closing log line
`ctx`: the frame as the loop holds it -- step (the InferStep), output and gt ([1,3,H,W] on the device), gt_yuv (the ground truth's
payload on the device), cut (the frame starts a sequence).  Everything of the project a grader calls is handed to it."""
import logging
import math
import os
import types

import torch

NR_KEYS = ("LOE", "LOE_50", "L_in", "L_out", "gain", "entropy_in", "entropy_out", "sat_out", "black_out")
COLOR_KEYS = ("UIQM", "UICM", "UISM", "UIConM", "UCIQE", "sigma_c", "con_l", "mu_s", "colorfulness", "mean_rgb")


class MetricTable:
    """One row per frame, an int64 half (exact sums) and a float64 half, in two device slots of `chunk` rows used in turn, each
    with a pinned host twin.  Columns first: `tab.ints(name, width)` / `tab.floats(name, width)` -> the slice of that half's row,
    of a device row and of a read-back row alike; then `build()`.  `row(frame)` -> the device row (ri, rf) the frame's kernels
    write into.  `advance(frames_done)` after every frame: a full chunk is copied to its host twin behind the kernels, and the
    chunk before it is read -- never the one just copied, so the host keeps running ahead of the device.  `finish()` copies the
    tail and reads everything left.  Both return the rows read, [(frame, ri, rf)] as lists, in frame order, each frame once."""

    def __init__(self, dev, chunk):
        self.dev, self.chunk = dev, int(chunk)
        self.names, self.width = set(), {torch.int64: 0, torch.float64: 0}
        self.slots = None
        self.pending = []                          # (slot, first frame, rows, event) of chunks copied but not yet read
        self.done, self.flushed = 0, 0             # frames written, frames copied to the host

    def _column(self, dtype, name, width):
        assert self.slots is None and name not in self.names, name
        self.names.add(name)
        start = self.width[dtype]
        self.width[dtype] = start + width
        return slice(start, start + width)

    def ints(self, name, width):
        return self._column(torch.int64, name, width)

    def floats(self, name, width):
        return self._column(torch.float64, name, width)

    def build(self):
        halves = [(self.chunk, w, dt) for dt, w in self.width.items()]
        self.slots = [[torch.zeros((r, w), dtype=dt, device=self.dev) for r, w, dt in halves] for _ in range(2)]
        self.host = [[torch.zeros((r, w), dtype=dt).pin_memory() for r, w, dt in halves] for _ in range(2)]
        return self

    def row(self, frame):
        ti, tf = self.slots[(frame // self.chunk) & 1]
        return ti[frame % self.chunk], tf[frame % self.chunk]

    def _flush(self, first, rows):
        slot = (first // self.chunk) & 1
        for h, d in zip(self.host[slot], self.slots[slot]):
            h.copy_(d, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self.pending.append((slot, first, rows, event))
        self.flushed = first + rows

    def _drain(self, keep):
        out = []
        while len(self.pending) > keep:
            slot, first, rows, event = self.pending.pop(0)
            event.synchronize()
            ri, rf = (h[:rows].tolist() for h in self.host[slot])
            out.extend((first + k, ri[k], rf[k]) for k in range(rows))
        return out

    def advance(self, frames_done):
        self.done = frames_done
        if frames_done - self.flushed < self.chunk:
            return []
        self._flush(self.flushed, self.chunk)
        return self._drain(1)

    def finish(self):
        if self.done > self.flushed:
            self._flush(self.flushed, self.done - self.flushed)
        return self._drain(0)


def _psnr_of(sq, n):
    return float("inf") if sq == 0 else 10.0 * math.log10(255.0 ** 2 * n / sq)


class RgbGrader:
    """PSNR (an exact integer sum) and SSIM of the output against the ground truth; with `lpips` (the model of
    zero-tig_amd/lpips.py) LPIPS as five layer sums, added on the host; with `hist_match` (f(output, gt) -> the matched frame)
    the same numbers of the matched frame as *_HM."""

    def __init__(self, tab, ops, npix, hist_match=None, lpips=None):
        self.ops, self.npix, self.hist_match, self.lpips = ops, npix, hist_match, lpips
        self.passes, self.tot = [], {}             # the output itself, then the matched frame; key -> sum over the frames
        for sfx in ("", "_HM") if hist_match else ("",):
            keys = [k + sfx for k in ("PSNR", "SSIM") + (("LPIPS",) if lpips else ())]
            self.passes.append(types.SimpleNamespace(
                matched=bool(sfx), sq=tab.ints("sq" + sfx, 1), ssim=tab.floats("ssim" + sfx, 1),
                lpips=tab.floats("lpips" + sfx, 5) if lpips else None, keys=keys,
                line="NUM: %d, " + ", ".join(k + ": %.3f" for k in keys), total_line=", ".join("Total " + k + ": %.3f" for k in keys)))
            self.tot.update(dict.fromkeys(keys, 0.0))

    def launch(self, ctx, ri, rf):
        gt_feat = None
        for p in self.passes:
            x = self.hist_match(ctx.output, ctx.gt) if p.matched else ctx.output
            self.ops.sqdiff_u8(x, ctx.gt, out=ri[p.sq])
            self.ops.ssim_u8_dev(x, ctx.gt, out=rf[p.ssim])
            if p.lpips is not None:                # the ground truth's features serve both passes
                gt_feat = self.lpips.features(ctx.gt) if gt_feat is None else gt_feat
                self.lpips.distance_dev(self.lpips.features(x), gt_feat, rf[p.lpips])

    def read(self, n, rec, ri, rf):
        tot = self.tot
        for p in self.passes:
            values = [_psnr_of(ri[p.sq][0], self.npix), rf[p.ssim][0]]
            if p.lpips is not None:
                a = rf[p.lpips]
                values.append((((a[0] + a[1]) + a[2]) + a[3]) + a[4])
            for k, x in zip(p.keys, values):
                tot[k] += x
                rec[k] = x
            logging.info(p.line, n, *values)
            logging.info(p.total_line, *[tot[k] / n for k in p.keys])

    def summary(self, result):
        for k, x in self.tot.items():
            result["Total_" + k] = x / max(result["images"], 1)


class PlaneGrader:
    """the SSE and SSIM of the three planes of the denoise payload against the ground truth's, which has its layout `fmt`;
    fmt None: the layouts differ, every field is null"""

    def __init__(self, tab, ops, fmt):
        self.ops, self.fmt = ops, fmt
        if fmt is not None:
            self.sse, self.ssim = tab.ints("plane_sse", 3), [tab.floats("plane_ssim_" + name, 1) for name in "YUV"]
        self.sse_tot, self.ssim_tot = [0, 0, 0], [0.0, 0.0, 0.0]

    def launch(self, ctx, ri, rf):
        if self.fmt is not None:
            self.ops.yuv_sse(ctx.step.yuv[1], ctx.gt_yuv, self.fmt, out=ri[self.sse])
            for p in range(3):
                self.ops.ssim_plane(ctx.step.yuv[1], ctx.gt_yuv, self.fmt, p, out=rf[self.ssim[p]])

    def read(self, n, rec, ri, rf):
        if self.fmt is None:
            rec.update(SSE=None, SSIM_Y=None, SSIM_U=None, SSIM_V=None)
            return
        sse, sp = ri[self.sse], [rf[s][0] for s in self.ssim]
        for p in range(3):
            self.sse_tot[p] += sse[p]
            self.ssim_tot[p] += sp[p]
        rec.update(SSE=sse, SSIM_Y=sp[0], SSIM_U=sp[1], SSIM_V=sp[2])
        logging.info("NUM: %d, SSE_Y: %d, SSE_U: %d, SSE_V: %d, SSIM_Y: %.3f, SSIM_U: %.3f, SSIM_V: %.3f", n, *sse, *sp)

    def summary(self, result):
        if self.fmt is None:
            return
        fmt, frames = self.fmt, result["images"]
        hc, wc = fmt.chroma_shape
        samples = [fmt.H * fmt.W, hc * wc, hc * wc]
        m = (1 << fmt.depth) - 1
        planes = {"depth": fmt.depth, "ss": fmt.ss, "samples": samples, "SSE": self.sse_tot}
        for p, name in enumerate("YUV"):
            planes["PSNR_" + name] = 10.0 * math.log10(m * m * samples[p] * frames / self.sse_tot[p]) if self.sse_tot[p] else None
        for p, name in enumerate("YUV"):
            planes["SSIM_" + name] = self.ssim_tot[p] / max(frames, 1)
        result["planes"] = planes


class TemporalGrader:
    """--tc 1: `tc` is the `TemporalConsistency`, or None when the frame is too small for it: every field is null.
    `from_output`: the flows come from the output itself (--noref 1, ctx.gt is the output), so there are no ground-truth
    numbers.  `meta`: the "scale" and "raft" of the summary; `extra`: what follows its numbers (viz, flo_dir).  `flags`: per
    frame, whether it was graded as a pair with the frame before it."""

    def __init__(self, tab, tc, from_output, meta, extra):
        self.tc, self.from_output, self.meta, self.extra = tc, from_output, meta, extra
        if tc is not None:
            self.n, self.sums = tab.ints("tc_valid", 2), tab.floats("tc_sums", 6)
        self.flags = []
        # valid pixels, the three sums of the output and of the ground truth, sum of (MABD - MABD_gt)^2, all over the pairs
        self.tot = {"n": 0, "out": [0.0, 0.0, 0.0], "gt": [0.0, 0.0, 0.0], "mabd_sq": 0.0}

    def launch(self, ctx, ri, rf):
        if self.tc is not None:
            if ctx.cut:                            # frame 0 and every scene cut: a pair never spans two sequences
                self.tc.reset()
            self.flags.append(self.tc.push(ctx.output, ctx.gt, ri[self.n], rf[self.sums]))

    def read(self, n, rec, ri, rf):
        rec["TC"] = None                           # the first frame of a sequence has no partner
        if self.tc is None or not self.flags[n - 1]:
            return
        tot, px = self.tot, self.tc.h * self.tc.w
        nv, o3, g3 = ri[self.n][0], rf[self.sums][0:3], None if self.from_output else rf[self.sums][3:6]
        tot["n"] += nv
        for q in range(3):
            tot["out"][q] += o3[q]
        rec["TC"] = {"N": nv, "out": o3, "gt": g3}
        e_warp = o3[0] / (3 * nv) if nv else float("nan")
        if g3 is None:
            logging.info("NUM: %d, TC valid: %d, E_warp: %.6f, MABD: %.6f (flows from the output)", n, nv, e_warp, o3[2] / (3 * px))
            return
        for q in range(3):
            tot["gt"][q] += g3[q]
        tot["mabd_sq"] += (o3[2] / (3 * px) - g3[2] / (3 * px)) ** 2
        logging.info("NUM: %d, TC valid: %d, E_warp: %.6f (gt %.6f), MABD: %.6f (gt %.6f)", n, nv, e_warp,
                     g3[0] / (3 * nv) if nv else float("nan"), o3[2] / (3 * px), g3[2] / (3 * px))

    def summary(self, result):
        result["temporal"] = None
        if self.tc is None:
            return
        tc, tot = self.tc, self.tot
        pairs, px = sum(self.flags), tc.h * tc.w
        te = {"scale": self.meta["scale"], "size": [tc.w, tc.h], "pairs": pairs, "raft": self.meta["raft"],
              "valid_share": tot["n"] / (pairs * px) if pairs else None}
        for sfx, s3 in (("", tot["out"]), ("_gt", tot["gt"])):
            te["E_warp" + sfx] = s3[0] / (3 * tot["n"]) if tot["n"] else None
            te["E_static" + sfx] = s3[1] / (3 * pairs * px) if pairs else None
            te["MABD" + sfx] = s3[2] / (3 * pairs * px) if pairs else None
        te["MABD_mse"] = tot["mabd_sq"] / pairs if pairs else None
        if self.from_output:
            te.update(E_warp_gt=None, E_static_gt=None, MABD_gt=None, MABD_mse=None, flow_from="output")
        te.update(self.extra)
        result["temporal"] = te
        logging.info("temporal (scale %d, %d pairs): %s", te["scale"], pairs,
                     ", ".join("%s: %s" % (k, "null" if te[k] is None else "%.6g" % te[k]) for k in
                               ("valid_share", "E_warp", "E_warp_gt", "E_static", "E_static_gt", "MABD", "MABD_gt", "MABD_mse")))


class TemporalPictures:
    """--tc_viz / --tc_flo_dir, after the temporal grader's launch: `viz` = (Y4MWriter, its format, radius, gain):
    one picture per frame, of the pair or of the frame alone, rendered in float and encoded by the kernel of the enhance stream;
    `flo` = (FloWriter, directory): the two flows of every graded pair.  Either may be None."""

    def __init__(self, ops, tc, dev, viz, flo):
        self.ops, self.tc, self.viz, self.flo = ops, tc, viz, flo
        if viz is not None:
            self.rgb = torch.empty((1, 3, 2 * tc.h, 2 * tc.w), dtype=torch.float32, device=dev)
            self.yuv = torch.empty(viz[1].frame_bytes, dtype=torch.uint8, device=dev)

    def submit(self, frame, paired):
        ops, tc = self.ops, self.tc
        if self.viz is not None:
            writer, fmt, radius, gain = self.viz
            tc.viz(self.rgb, "out", radius, gain)
            writer.submit(ops.rgb_f32_to_yuv(self.rgb, fmt, out=self.yuv))
        if self.flo is not None and paired:
            for flow, name in ((tc.fb, "bwd"), (tc.ff, "fwd")):
                self.flo[0].submit(os.path.join(self.flo[1], "%06d_%s.flo" % (frame, name)), ops.flow_pack(flow, tc.h, tc.w))


def loe50_grid(H, W):
    """the sample grid of LOE_50: the short side becomes 50, the other side keeps the aspect, each rounded half up"""
    m = min(H, W)
    return (100 * H + m) // (2 * m), (100 * W + m) // (2 * m)


def noref_values(full, ents, sub):
    """the per-frame numbers of --noref 1 from what `Ops.noref` returns on the full grid (six integers `full`, two entropies
    `ents`) and on the LOE_50 grid (`sub`): [Ns, S_loe, S_a, S_b, n_sat, n_black]"""
    ns = full[0]
    l_in, l_out = full[2] / ns, full[3] / ns
    return {"LOE": full[1] / (ns * (ns - 1)) if ns > 1 else None, "LOE_50": sub[1] / sub[0], "L_in": l_in, "L_out": l_out,
            "gain": l_out / l_in if full[2] else None, "entropy_in": ents[0], "entropy_out": ents[1], "sat_out": full[4] / ns,
            "black_out": full[5] / ns}


def color_values(ints, floats, block):
    """the colour measures of a frame from what `Ops.color_stats` returns for blocks of `block` pixels, 18 integers and
    7 floats as include/zerotig_hip.h lists them; float64; None where a denominator is 0 (one pixel: nothing is left after the
    trimming; a frame smaller than a block)"""
    n, nblk = ints[0], ints[1]
    assert n >= 1 and 0 <= nblk * block * block <= n, (n, nblk, block)
    s1_rg, s2_rg, t_rg, s1_yb, s2_yb, t_yb, kept, k01, k99 = ints[5:14]
    sum_c, sum_c2, sum_s, e_r, e_g, e_b, a = floats
    uicm = None
    if kept:                                       # the spread of all the pixels about the trimmed mean, as in the paper
        mu_rg, mu_yb = t_rg / kept, t_yb / (2 * kept)
        var_rg = s2_rg / n - 2.0 * mu_rg * s1_rg / n + mu_rg * mu_rg
        var_yb = s2_yb / (4 * n) - 2.0 * mu_yb * s1_yb / (2 * n) + mu_yb * mu_yb
        uicm = -0.0268 * math.hypot(mu_rg, mu_yb) + 0.1586 * math.sqrt(max(var_rg + var_yb, 0.0))
    uism = (0.299 * e_r + 0.587 * e_g + 0.114 * e_b) / nblk if nblk else None
    uiconm = -a / nblk if nblk else None
    uiqm = None if uicm is None or uism is None else 0.0282 * uicm + 0.2953 * uism + 3.5753 * uiconm
    sigma_c = math.sqrt(max(sum_c2 / n - (sum_c / n) ** 2, 0.0)) / 255.0
    con_l, mu_s = (k99 - k01) / 1000.0, sum_s / n
    m_rg, m_yb = s1_rg / n, s1_yb / (2 * n)       # Hasler and Suesstrunk: the plain means and variances
    v_rg, v_yb = s2_rg / n - m_rg * m_rg, s2_yb / (4 * n) - m_yb * m_yb
    return {"UIQM": uiqm, "UICM": uicm, "UISM": uism, "UIConM": uiconm,
            "UCIQE": 0.4680 * sigma_c + 0.2745 * con_l + 0.2576 * mu_s, "sigma_c": sigma_c, "con_l": con_l, "mu_s": mu_s,
            "colorfulness": math.sqrt(max(v_rg + v_yb, 0.0)) + 0.3 * math.hypot(m_rg, m_yb), "mean_rgb": [s / n for s in ints[2:5]]}


class ColorMeans:
    """per key of COLOR_KEYS the sum of the frames' values and the number of frames that have one (`NorefGrader`'s rule)"""

    def __init__(self):
        self.tot = dict.fromkeys(COLOR_KEYS, 0.0)
        self.tot["mean_rgb"] = [0.0, 0.0, 0.0]
        self.count = dict.fromkeys(COLOR_KEYS, 0)

    def add(self, v):
        for key in COLOR_KEYS:
            if v[key] is None:
                continue
            if key == "mean_rgb":
                self.tot[key] = [t + x for t, x in zip(self.tot[key], v[key])]
            else:
                self.tot[key] += v[key]
            self.count[key] += 1

    def means(self):
        out = {}
        for key in COLOR_KEYS:
            c, t = self.count[key], self.tot[key]
            out[key] = None if not c else [x / c for x in t] if key == "mean_rgb" else t / c
        return out


def color_text(v):
    return ", ".join("%s: %s" % (k, "null" if v[k] is None else "%.4f" % v[k]) for k in ("UIQM", "UICM", "UISM", "UIConM", "UCIQE",
                                                                                       "colorfulness"))


class ColorGrader:
    """--color 1: one `Ops.color_stats` with blocks of `block` pixels per graded frame; `which` names the frames, in
    the order of the log: "out" the denoise result, "in" the decoded input as the network saw it (step.x), "gt" the ground truth"""

    def __init__(self, tab, ops, block, which):
        self.ops, self.block, self.which = ops, block, tuple(which)
        self.cols = {w: (tab.ints("color_" + w, 18), tab.floats("color_" + w + "_sums", 7)) for w in self.which}
        self.means = {w: ColorMeans() for w in self.which}
        self.blocks = None                         # [k2, k1] of the frames, known from the first one

    def launch(self, ctx, ri, rf):
        frames = {"out": ctx.output, "in": ctx.step.x, "gt": ctx.gt}
        if self.blocks is None:
            self.blocks = [int(ctx.output.shape[2]) // self.block, int(ctx.output.shape[3]) // self.block]
        for w in self.which:
            ci, cf = self.cols[w]
            self.ops.color_stats(frames[w], self.block, out_i=ri[ci], out_f=rf[cf])

    def read(self, n, rec, ri, rf):
        rec["color"] = {}
        for w in self.which:
            ci, cf = self.cols[w]
            v = color_values(ri[ci], rf[cf], self.block)
            self.means[w].add(v)
            rec["color"][w] = dict(v, ints=ri[ci], sums=rf[cf])
            logging.info("NUM: %d, color %s: %s", n, w, color_text(v))

    def summary(self, result):
        co = {"block": self.block, "graded": "denoise", "blocks": self.blocks, "out": None, "in": None, "gt": None}
        co.update({w: self.means[w].means() for w in self.which})
        result["color"] = co
        logging.info("colour (%d frames, blocks of %d): %s", result["images"], self.block,
                     "; ".join("%s %s" % (w, color_text(co[w])) for w in self.which))


_NIQE_TABLES = []


def niqe_tables():
    """-> (win float32 [7], r_gam, c1, c2 float64 [9801]) as include/zerotig_hip.h defines them, made in float64; made once"""
    import numpy as np
    if not _NIQE_TABLES:
        k = np.arange(-3, 4, dtype=np.float64)
        win = np.exp(-k * k / (2.0 * (7.0 / 6.0) ** 2))
        lg = math.lgamma
        alpha = [0.2 + 0.001 * i for i in range(9801)]
        r_gam = np.array([math.exp(2.0 * lg(2.0 / a) - lg(1.0 / a) - lg(3.0 / a)) for a in alpha], dtype=np.float64)
        c1 = np.array([math.sqrt(math.exp(lg(1.0 / a) - lg(3.0 / a))) for a in alpha], dtype=np.float64)
        c2 = np.array([math.exp(lg(2.0 / a) - lg(1.0 / a)) for a in alpha], dtype=np.float64)
        assert bool(np.all(np.diff(r_gam) > 0))
        _NIQE_TABLES.extend([(win / win.sum()).astype(np.float32), r_gam, c1, c2])
    return tuple(_NIQE_TABLES)


def niqe_features(sums_i, sums_f):
    """the fits of the header in numpy float64, for the fitting of a model: what `Ops.niqe_block_sums` returns, read back
    ([2,n,10], [2,n,16]) -> float64 [n,36], NaN where a fit has no value"""
    import numpy as np
    _, r_gam, c1, c2 = niqe_tables()
    si, sf = np.asarray(sums_i, dtype=np.int64), np.asarray(sums_f, dtype=np.float64)
    n = si.shape[1]
    si, sf = si.reshape(2, n, 5, 2), sf[:, :, :15].reshape(2, n, 5, 3)
    px = np.array([9216.0, 2304.0]).reshape(2, 1, 1)
    with np.errstate(all="ignore"):
        l, r = np.sqrt(sf[..., 0] / si[..., 0]), np.sqrt(sf[..., 1] / si[..., 1])
        gh = l / r
        rhat = (sf[..., 2] / px) ** 2 / ((sf[..., 0] + sf[..., 1]) / px)
        rn = rhat * (gh * gh * gh + 1.0) * (gh + 1.0) / ((gh * gh + 1.0) * (gh * gh + 1.0))
        ok = (si[..., 0] > 0) & (si[..., 1] > 0) & np.isfinite(rn)
        j = np.searchsorted(r_gam, np.where(ok, rn, 1.0), side="left")
        lo, hi = np.clip(j - 1, 0, 9800), np.clip(j, 0, 9800)
        pos = np.where((r_gam[lo] - rn) ** 2 <= (r_gam[hi] - rn) ** 2, lo, hi)
        alpha = np.where(ok, 0.2 + 0.001 * pos, np.nan)
        bl, br = np.where(ok, l * c1[pos], np.nan), np.where(ok, r * c1[pos], np.nan)
        mean = (br - bl) * c2[pos]
    feat = np.empty((n, 36), dtype=np.float64)
    for s in range(2):
        feat[:, 18 * s], feat[:, 18 * s + 1] = alpha[s, :, 0], (bl[s, :, 0] + br[s, :, 0]) / 2.0
        for f in range(1, 5):
            feat[:, 18 * s + 4 * f - 2:18 * s + 4 * f + 2] = np.stack([alpha[s, :, f], mean[s, :, f], bl[s, :, f], br[s, :, f]], axis=1)
    return feat


def _triu_to_full(tri, n=36):
    import numpy as np
    full = np.zeros((n, n), dtype=np.float64)
    full[np.triu_indices(n)] = np.asarray(tri, dtype=np.float64)
    return full + np.triu(full, 1).T


def niqe_value(ints, floats, model):
    """NIQE of a frame from what `Ops.niqe_frame` returns, 38 integers and 738 floats as include/zerotig_hip.h lists
    them, against the pristine `model`; float64 on the host; None when fewer than two rows are valid or a column has no finite value"""
    import numpy as np
    nv, count = ints[1], np.asarray(ints[2:38], dtype=np.float64)
    if nv < 2 or bool(np.any(count == 0)):
        return None
    mu_d = np.asarray(floats[0:36], dtype=np.float64) / count
    cov_d = _triu_to_full(floats[72:738]) / (nv - 1)
    d = model.mu - mu_d
    q = float(d @ np.linalg.pinv((model.cov + cov_d) / 2.0) @ d)
    return math.sqrt(max(q, 0.0)) if math.isfinite(q) else None


class NiqeModel:
    """the pristine model of NIQE: `mu` float64 [36], `cov` float64 [36,36]; `name` says where it came from"""

    def __init__(self, mu, cov, name="model"):
        import numpy as np
        mu, cov = np.asarray(mu, dtype=np.float64), np.asarray(cov, dtype=np.float64)
        assert mu.shape in ((36,), (1, 36)) and cov.shape == (36, 36), (mu.shape, cov.shape)
        self.mu, self.cov, self.name = mu.reshape(36), cov, name

    @classmethod
    def load(cls, path):
        """.npz with mu_pris_param / cov_pris_param (the Python ports' file, and `save`'s); .mat with mu_prisparam / cov_prisparam
        (the MATLAB release's modelparameters.mat), which needs scipy"""
        import numpy as np
        if str(path).lower().endswith(".mat"):
            try:
                from scipy.io import loadmat
            except ImportError:
                raise ValueError("%s: reading a .mat model needs scipy, which cannot be imported here; convert it to .npz with the "
                                 "keys mu_pris_param [36] and cov_pris_param [36,36]" % path)
            data, keys = loadmat(path), ("mu_prisparam", "cov_prisparam")
            found = sorted(k for k in data if not k.startswith("__"))
        else:
            data, keys = np.load(path), ("mu_pris_param", "cov_pris_param")
            found = sorted(data.files)
        if keys[0] not in found or keys[1] not in found:
            raise ValueError("%s: a NIQE model holds %s and %s; the file holds %s" % (path, keys[0], keys[1], found))
        mu, cov = np.asarray(data[keys[0]], dtype=np.float64), np.asarray(data[keys[1]], dtype=np.float64)
        if mu.shape not in ((36,), (1, 36)) or cov.shape != (36, 36):
            raise ValueError("%s: %s must be [36] or [1,36] and %s [36,36]; they are %s and %s (the file holds %s)"
                             % (path, keys[0], keys[1], list(mu.shape), list(cov.shape), found))
        return cls(mu, cov, os.path.basename(str(path)))

    def save(self, path):
        import numpy as np
        with open(path, "wb") as fh:               # a file object: numpy adds no suffix of its own
            np.savez(fh, mu_pris_param=self.mu.reshape(1, 36), cov_pris_param=self.cov)

    @staticmethod
    def select(sums_f):
        """the blocks of one frame that go into a model (paper section 3): sharpness S_sigma / 9216 at scale 1 greater than 0.75
        times the frame's largest -> bool [n]"""
        import numpy as np
        sharp = np.asarray(sums_f, dtype=np.float64)[0, :, 15] / 9216.0
        return sharp > 0.75 * sharp.max()

    @classmethod
    def fit(cls, frames, name="fitted"):
        """`frames`: per frame what `Ops.niqe_block_sums` returned, read back, (sums_i [2,n,10], sums_f [2,n,16]).  The sharp
        blocks of every frame (`select`), their 36 features by `niqe_features`; mu = the mean of each column over its finite
        values, cov = the sample covariance of the rows that are all finite about their own mean."""
        import numpy as np
        rows = [niqe_features(si, sf)[cls.select(sf)] for si, sf in frames]
        feat = np.concatenate(rows, axis=0) if rows else np.zeros((0, 36))
        valid = feat[np.all(np.isfinite(feat), axis=1)]
        if valid.shape[0] < 2 or not bool(np.all(np.any(np.isfinite(feat), axis=0))):
            raise ValueError("a NIQE model needs at least two sharp blocks whose features are all finite; got %d of %d"
                             % (valid.shape[0], feat.shape[0]))
        model = cls(np.nanmean(feat, axis=0), np.cov(valid, rowvar=False, ddof=1), name)
        model.blocks = (int(valid.shape[0]), int(feat.shape[0]))
        return model


class NiqeGrader:
    """--niqe MODEL: one `Ops.niqe_frame` per graded frame; `which` names the frames as `ColorGrader`'s does.  A frame
    with fewer than two whole blocks is not graded: its cells stay zero, which `niqe_value` reads as no value."""

    def __init__(self, tab, ops, model, which):
        self.ops, self.model, self.which = ops, model, tuple(which)
        self.cols = {w: (tab.ints("niqe_" + w, 38), tab.floats("niqe_" + w + "_sums", 738)) for w in self.which}
        self.tot, self.count = dict.fromkeys(self.which, 0.0), dict.fromkeys(self.which, 0)
        self.blocks = None                         # [k2, k1] of the frames, known from the first one

    def launch(self, ctx, ri, rf):
        frames = {"out": ctx.output, "in": ctx.step.x, "gt": ctx.gt}
        if self.blocks is None:
            self.blocks = [int(ctx.output.shape[2]) // 96, int(ctx.output.shape[3]) // 96]
        if self.blocks[0] * self.blocks[1] < 2:
            return
        for w in self.which:
            ci, cf = self.cols[w]
            self.ops.niqe_frame(frames[w], out_i=ri[ci], out_f=rf[cf])

    def read(self, n, rec, ri, rf):
        rec["niqe"] = {"out": None, "in": None, "gt": None, "valid_blocks": {}}
        for w in self.which:
            ci, cf = self.cols[w]
            v = niqe_value(ri[ci], rf[cf], self.model)
            if v is not None:                      # the means count only the frames that have a value
                self.tot[w] += v
                self.count[w] += 1
            rec["niqe"][w] = v
            rec["niqe"]["valid_blocks"][w] = ri[ci][1]
        logging.info("NUM: %d, NIQE %s", n, ", ".join("%s: %s" % (w, "null" if rec["niqe"][w] is None else "%.4f" % rec["niqe"][w])
                                                       for w in self.which))

    def summary(self, result):
        nq = {"model": self.model.name, "blocks": self.blocks, "graded": "denoise", "out": None, "in": None, "gt": None,
              "frames_with_value": dict(self.count)}
        nq.update({w: self.tot[w] / self.count[w] if self.count[w] else None for w in self.which})
        result["niqe"] = nq
        logging.info("NIQE (%d frames, model %s): %s", result["images"], self.model.name,
                     ", ".join("%s: %s" % (w, "null" if nq[w] is None else "%.4f" % nq[w]) for w in self.which))


class NorefGrader:
    """--noref 1: `Ops.noref` of the decoded input as the network saw it (step.x) against the output, on the full
    grid and on the LOE_50 grid `grid50`"""

    def __init__(self, tab, ops, grid50):
        self.ops, self.grid50 = ops, grid50
        self.full, self.ents = tab.ints("noref", 6), tab.floats("noref_entropy", 2)
        self.sub, self.ents_sub = tab.ints("noref_50", 6), tab.floats("noref_50_entropy", 2)     # its entropies are not reported
        # per key the sum of the frames' values and the number of frames that have one; sum of S_a and of S_b
        self.tot, self.count, self.s = dict.fromkeys(NR_KEYS, 0.0), dict.fromkeys(NR_KEYS, 0), [0, 0]

    def launch(self, ctx, ri, rf):
        self.ops.noref(ctx.step.x, ctx.output, out_i=ri[self.full], out_f=rf[self.ents])
        self.ops.noref(ctx.step.x, ctx.output, grid=self.grid50, out_i=ri[self.sub], out_f=rf[self.ents_sub])

    def read(self, n, rec, ri, rf):
        tot, count, s = self.tot, self.count, self.s
        full, sub = ri[self.full], ri[self.sub]
        v = noref_values(full, rf[self.ents], sub)
        for key in NR_KEYS:
            if v[key] is not None:
                tot[key] += v[key]
                count[key] += 1
        s[0] += full[2]
        s[1] += full[3]
        rec["noref"] = dict(v, ints=full, ints_50=sub)
        logging.info("NUM: %d, " + ", ".join(key + ": %s" for key in NR_KEYS), n,
                     *["null" if v[key] is None else "%.4f" % v[key] for key in NR_KEYS])
        logging.info("Total LOE: %s, Total LOE_50: %.4f, Total L_out: %.4f, Total gain: %s",
                     "%.4f" % (tot["LOE"] / count["LOE"]) if count["LOE"] else "null", tot["LOE_50"] / n, tot["L_out"] / n,
                     "%.4f" % (s[1] / s[0]) if s[0] else "null")

    def summary(self, result):
        nr = dict({"graded": "denoise"}, **{k: self.tot[k] / self.count[k] if self.count[k] else None for k in NR_KEYS})
        nr["gain"] = self.s[1] / self.s[0] if self.s[0] else None               # of the stream: sum S_b / sum S_a
        result["noref"] = nr
        logging.info("no-reference (%d frames, the denoise result against the decoded input): %s", result["images"],
                     ", ".join("%s: %s" % (k, "null" if nr[k] is None else "%.6g" % nr[k]) for k in NR_KEYS))
