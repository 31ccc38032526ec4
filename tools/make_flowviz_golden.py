#!/usr/bin/env python3
"""Make tests/golden/g13_flowviz.npz: what the reference's `utils/flow_viz.py` and `utils/frame_utils.py` produce for the flows of
tests/test_flowviz.py (`golden_inputs`).  Runs where the reference tree is (ZT_REFERENCE, default /root/reference); the two modules
are imported by path with an empty `cv2` in their way, nothing of them is copied, only their outputs are stored.

Before the file is written, every gate the tests hold the kernels to is asserted on the numpy float32 restatement
(`check_golden` of tests/test_flowviz.py): if the restatement cannot meet a gate, no kernel that equals it bit for bit can."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ZT_REFERENCE", "/root/reference")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
F = np.float32


def _by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    cv2 = types.ModuleType("cv2")
    cv2.setNumThreads = lambda n: None
    cv2.ocl = types.SimpleNamespace(setUseOpenCL=lambda b: None)
    sys.modules.setdefault("cv2", cv2)
    ref_viz = _by_path("ref_flow_viz", os.path.join(REF, "utils", "flow_viz.py"))
    ref_io = _by_path("ref_frame_utils", os.path.join(REF, "utils", "frame_utils.py"))
    import test_flowviz as tf
    from test_temporal import _case

    flows = tf.golden_inputs()
    den6 = F(6) + F(1e-5)
    g = {"wheel": ref_viz.make_colorwheel().astype(np.uint8), "crc_noise": np.int64(tf.crc(flows["noise"])),
         "crc_smooth": np.int64(tf.crc(flows["smooth"])), "small_flow": flows["small"], "compass_flow": flows["compass"]}
    assert (ref_viz.make_colorwheel() == g["wheel"]).all()
    for name in ("noise", "smooth", "compass"):
        fl = flows[name]
        g[name + "_image"] = ref_viz.flow_to_image(fl)
        un = fl / den6
        g[name + "_colors6"] = ref_viz.flow_uv_to_colors(un[..., 0], un[..., 1])
    g["small_image_bgr"] = ref_viz.flow_to_image(flows["small"], convert_to_bgr=True)
    g["small_image"] = ref_viz.flow_to_image(flows["small"])
    g["smooth_image_clip2"] = ref_viz.flow_to_image(flows["smooth"], clip_flow=2.0)
    # the .flo bytes of the backward flow of test_temporal.py's 33 x 130 window
    _, _, fb, _, oy, ox, _ = _case("smooth", (33, 130, 40, 136))
    flow = np.ascontiguousarray(fb[:, oy:oy + 33, ox:ox + 130].transpose(1, 2, 0))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "a.flo")
        ref_io.writeFlow(path, flow)
        data = open(path, "rb").read()
        assert ref_io.readFlow(path).tobytes() == flow.tobytes()
    g["flo_bytes"] = np.frombuffer(data, np.uint8)
    assert all(v.dtype == np.uint8 for k, v in g.items() if k.endswith(("_image", "_colors6", "_bgr", "_clip2", "_colors")))

    # ---- the gates, on the restatement alone
    def render(flow, radius, bgr):
        r = tf.np_radmax((flow.transpose(2, 0, 1),), (slice(None), slice(None))) if radius is None else radius
        return tf.np_flow_levels(np.ascontiguousarray(flow[..., 0]), np.ascontiguousarray(flow[..., 1]), r, bgr)
    gf = dict(flows)
    tf.check_golden(render, g, gf)
    assert np.array_equal(tf.wheel_levels(), g["wheel"])
    tf.gate(render(np.clip(flows["smooth"], 0, 2.0), None, False), g["smooth_image_clip2"], "smooth clip_flow=2.0")
    out = os.path.join(ROOT, "tests", "golden", "g13_flowviz.npz")
    np.savez_compressed(out, **g)
    print("wrote %s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
