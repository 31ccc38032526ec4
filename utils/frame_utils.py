"""Drop-in for the `.flo` half of the reference's `utils/frame_utils.py`, over zero-tig_amd/flowio.py.  KITTI .png flow and .pfm stay
out of scope."""
import importlib

import numpy as np

_flowio = importlib.import_module("zero-tig_amd.flowio")
TAG_CHAR = np.array([_flowio.TAG], np.float32)


def readFlow(fn):
    """a Middlebury .flo file -> float32 [H, W, 2]; unlike the reference, which prints and returns None, a file that is not one
    raises ValueError"""
    return _flowio.read_flo(fn)


def writeFlow(filename, uv, v=None):
    """uv [H, W, 2], or u and v [H, W] each"""
    if v is None:
        uv = np.asarray(uv)
        assert uv.ndim == 3 and uv.shape[2] == 2, uv.shape
    else:
        u, v = np.asarray(uv), np.asarray(v)
        assert u.shape == v.shape and u.ndim == 2, (u.shape, v.shape)
        uv = np.stack([u, v], axis=-1)
    _flowio.write_flo(filename, uv)
