"""LPIPS (VGG16, lpips 0.1, eval mode) on the HIP kernels: `lpips.LPIPS(net='vgg')` as the reference's evals.py:73-80, 92-98 calls it.

The weights are the user's file (`torch.save(lpips.LPIPS(net='vgg').state_dict(), 'lpips_vgg.pt')`); nothing is shipped or fetched.
precision "fp32": every conv through the exact fp32 kernel (parity mode); "bf16": bf16 activations and weights, fp32 accumulation --
conv1_1 / conv1_2 through zt_conv2d_nhwc_bf16, the eleven wide layers through zt_conv3x3_wide_bf16."""
import re

import torch

# torchvision vgg16.features: index of every conv, its (Cin, Cout); a 2x2 max pool sits in front of the convs listed in POOL_BEFORE;
# the LPIPS taps are the ReLU outputs of the convs in TAPS (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3)
CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_CH = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
           (512, 512), (512, 512), (512, 512))
POOL_BEFORE = (5, 10, 17, 24)
TAPS = (2, 7, 14, 21, 28)
TAP_CH = (64, 128, 256, 512, 512)


def resolve_state_dict(sd):
    """-> ([(weight, bias)] x 13, [lin weight [C]] x 5) from an `lpips.LPIPS(net='vgg').state_dict()` (`net.slice<k>.<idx>.*`,
    `lin<k>.model.1.weight` / `lins.<k>.model.1.weight`) or, for the convs, torchvision's `features.<idx>.*`.  A conv is found by
    the index suffix of its key and checked by shape; `scaling_layer.*` is ignored (the constants are lpips 0.1's).
    Raises ValueError naming the missing or misshapen layer and listing the keys that were found."""
    if not isinstance(sd, dict):
        raise ValueError("LPIPS weights: expected a state dict, got %s" % type(sd).__name__)
    keys = sorted(str(k) for k in sd)

    def fail(what):
        raise ValueError("LPIPS weights: %s; keys found: %s" % (what, ", ".join(keys) if keys else "(none)"))

    def find(pattern, shape, what):
        for k in keys:
            if re.fullmatch(pattern, k) and torch.is_tensor(sd[k]):
                if tuple(sd[k].shape) != shape:
                    fail("%s (%s) has shape %s, expected %s" % (what, k, tuple(sd[k].shape), shape))
                return sd[k].detach().to(torch.float32)
        fail("%s is missing" % what)

    convs = []
    for idx, (cin, cout) in zip(CONV_IDX, CONV_CH):
        stem = r"(?:.*\.)?(?:slice\d+|features)\.%d\." % idx
        convs.append((find(stem + "weight", (cout, cin, 3, 3), "conv weight of features[%d]" % idx),
                      find(stem + "bias", (cout,), "conv bias of features[%d]" % idx)))
    lins = []
    for k, c in enumerate(TAP_CH):
        lins.append(find(r"(?:.*\.)?(?:lin%d|lins\.%d)\.model\.1\.weight" % (k, k), (1, c, 1, 1), "lin%d weight" % k).reshape(c))
    return convs, lins


class LpipsVGG:
    def __init__(self, ops, state_dict, device, precision="fp32"):
        if precision not in ("fp32", "bf16"):
            raise ValueError("LPIPS precision must be 'fp32' or 'bf16', got %r" % (precision,))
        self.ops, self.device, self.precision = ops, torch.device(device), precision
        convs, lins = resolve_state_dict(state_dict)
        self.lin = [w.contiguous().to(self.device) for w in lins]
        self.layers = []
        for w, b in convs:
            w = w.contiguous().to(self.device)
            wdev = ops.repack_weight_bf16(w) if precision == "bf16" else ops.repack_weight(w)
            self.layers.append((wdev, b.contiguous().to(self.device), int(w.shape[1]), int(w.shape[0])))

    def features(self, img):
        """[1,3,H,W] fp32 in [0,1] on the device -> the five tap maps (NHWC, fp32 or bf16)."""
        from .ops import CV
        ops, bf = self.ops, self.precision == "bf16"
        img = img.detach().contiguous().float()
        x = CV(ops.lpips_prep(img, torch.bfloat16 if bf else torch.float32), 0, 3)
        taps = []
        for idx, (wdev, bias, cin, cout) in zip(CONV_IDX, self.layers):
            if idx in POOL_BEFORE:
                x = ops.maxpool2(x)
            if not bf:
                x = ops.conv2d(x, wdev, bias, cout, 3, 3, pad=(1, 1), act="relu")
            elif cin < 64 or cout < 128:
                x = ops.conv2d_bf16(x, wdev, bias, cout, 3, 3, pad=(1, 1), act="relu")
            else:
                x = ops.conv3x3_wide_bf16(x, wdev, bias, cout, relu=True)
            if idx in TAPS:
                taps.append(x)
        return taps

    def distance(self, fa, fb):
        """-> (LPIPS, [d_1 .. d_5]) as Python floats from two `features` results; one 40-byte read-back."""
        out = torch.empty(5, dtype=torch.float64, device=self.device)
        for l in range(5):
            self.ops.lpips_layer(fa[l], fb[l], self.lin[l], out[l:l + 1])
        d = [float(v) for v in out.cpu().tolist()]
        return ((((d[0] + d[1]) + d[2]) + d[3]) + d[4]), d

    def distance_dev(self, fa, fb, out5):
        """[d_1 .. d_5] of `distance` into `out5` (float64 [5] on the device, e.g. part of a table row); no read-back.  The
        caller's LPIPS is (((d_1 + d_2) + d_3) + d_4) + d_5, the order `distance` adds them in."""
        assert out5.dtype == torch.float64 and tuple(out5.shape) == (5,) and out5.is_contiguous(), (out5.dtype, tuple(out5.shape))
        for l in range(5):
            self.ops.lpips_layer(fa[l], fb[l], self.lin[l], out5[l:l + 1])
        return out5

    def __call__(self, a, b):
        return self.distance(self.features(a), self.features(b))[0]
