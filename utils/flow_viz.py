"""Drop-in for the reference's `utils/flow_viz.py` (the Middlebury colour wheel, Baker et al. 2007): the same names, numpy in, numpy
uint8 out, computed on the device by csrc/zt_flowviz.hip.  The arithmetic is fp32 and the angle a polynomial, so a
sample in ten thousand may differ from the reference's float64 / arctan2 result by one level; NaN, infinite and overflowing flows,
undefined there, are drawn black."""
import numpy as np
import torch

from . import utils as _utils

# the radius R with R + 1e-5f == 1 in float32: `flow_uv_to_colors` takes flows that are already scaled
_UNIT = np.float32(1) - np.float32(1e-5)
assert _UNIT + np.float32(1e-5) == np.float32(1)


def make_colorwheel():
    """-> float64 [55, 3], the wheel's levels 0..255 (the array the reference returns)"""
    return _utils._ops().flow_wheel().numpy().astype(np.float64)


def _on_device(u, v):
    u, v = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)
    assert u.ndim == 2 and u.shape == v.shape, (u.shape, v.shape)
    dev = torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(np.ascontiguousarray(np.stack([u, v])[None])).to(dev)


def flow_uv_to_colors(u, v, convert_to_bgr=False):
    """u, v [H, W], already divided by the largest radius -> uint8 [H, W, 3]"""
    flow = _on_device(u, v)
    return _utils._ops().flow_to_rgb(flow, radius=float(_UNIT), u8=True, bgr=convert_to_bgr).cpu().numpy()


def flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False):
    """flow_uv [H, W, 2] -> uint8 [H, W, 3], scaled by the flow's own largest radius.  `clip_flow` does what it does in the
    reference: np.clip(flow_uv, 0, clip_flow), which also removes every negative component."""
    uv = np.asarray(flow_uv)
    if uv.ndim != 3 or uv.shape[2] != 2:
        raise ValueError("flow_to_image: a flow is [H, W, 2]; got %s" % (uv.shape,))
    if clip_flow is not None:
        uv = uv.clip(0, clip_flow)
    flow = _on_device(uv[..., 0], uv[..., 1])
    return _utils._ops().flow_to_rgb(flow, u8=True, bgr=convert_to_bgr).cpu().numpy()
