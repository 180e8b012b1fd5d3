"""LPIPS (AlexNet) on the GPU from user-supplied weights: what the reference's ``RGBMetrics`` gets from torchmetrics'
``LearnedPerceptualImagePatchSimilarity`` (metrics.py:83-112), in HIP (csrc/lpips.hip).

The pretrained weights are not shipped and nothing is ever fetched: hand over the two files and the
``rgb_lpips`` entry is filled; without them it stays NaN.

Formulas, fixed here (torchmetrics' defaults: ``net_type="alex"``, ``normalize=False``, ``reduction="mean"`` -- the
reference's [0, 1] images go into the scaling layer as they are):

  * scaling layer: ``x' = (x - SHIFT) / SCALE`` per channel, applied BEFORE conv1's zero padding, so a padded tap is 0;
  * features: the five convolution + bias + ReLU layers of ``LAYERS``, a 3x3 max-pool with stride 2 (no padding, floor)
    in front of conv2 and in front of conv3;
  * per layer and pixel both channel vectors are unit-normalised, ``f / sqrt(EPS + sum_c f^2)`` with ``EPS`` inside the
    root (an all-zero pixel gives 0, not NaN); the squared difference is weighted by the layer's ``lin`` vector and
    summed over the channels; mean over the pixels; sum over the five layers.

Convolutions run in float32 on the exact f32-input matrix instruction with a fixed summation order; the pixel sums are
folded in float64 without atomics: the same input gives the same bits, and ``lpips(a, a)`` is exactly 0.  The value
stays on the device; nothing on the path synchronises with the host.  There is no backward pass (a metric, not a loss),
and no CPU path: without the library or a GPU the call raises.

    python -m qed_splatter_amd.lpips --pred A.png --gt B.png --weights alexnet.pth [lin_alex.pth]
"""
from __future__ import annotations

import argparse
import collections
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib as L

EPS = 1e-8
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (Cin, Cout, kernel, stride, padding) of conv1 .. conv5
LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
POOL_BEFORE = (1, 2)                       # a max-pool in front of conv2 and conv3
FEATURE_KEYS = (0, 3, 6, 8, 10)            # torchvision's AlexNet: features.{i}.{weight,bias}
MIN_SIDE = 31                              # below it nothing is left after conv1 and the two pools
ENV_VAR = "QED_LPIPS_WEIGHTS"


def conv_out(n: int, layer: int) -> int:
    _, _, k, s, p = LAYERS[layer]
    return (n + 2 * p - k) // s + 1


def pool_out(n: int) -> int:
    return (n - 3) // 2 + 1


def feature_sizes(H: int, W: int) -> List[Tuple[int, int]]:
    """(height, width) of the five feature maps of an H x W image."""
    out = []
    h, w = H, W
    for l in range(5):
        if l in POOL_BEFORE:
            h, w = pool_out(h), pool_out(w)
        h, w = conv_out(h, l), conv_out(w, l)
        out.append((h, w))
    return out


def _round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def pack_conv(weight: Tensor, layer: int) -> Tensor:
    """[Cout,Cin,k,k] -> the kernel's [Kp,Np] layout: row (kh * k + kw) * Cin + c, column = output channel, zero-padded
    to multiples of the K and N tiles (include/qed_splat.h: qed_lpips_conv)."""
    cin, cout, k, _, _ = LAYERS[layer]
    K = cin * k * k
    out = torch.zeros(_round_up(K, L.LPIPS_TILE_K), _round_up(cout, L.LPIPS_TILE_N), dtype=torch.float32,
                      device=weight.device)
    out[:K, :cout] = weight.to(torch.float32).permute(2, 3, 1, 0).reshape(K, cout)
    return out


def unpack_conv(packed: Tensor, layer: int) -> Tensor:
    """The inverse of ``pack_conv``: [Kp,Np] -> [Cout,Cin,k,k]."""
    cin, cout, k, _, _ = LAYERS[layer]
    return packed[:cin * k * k, :cout].reshape(k, k, cin, cout).permute(3, 2, 0, 1).contiguous()


def _read(path) -> Dict[str, Tensor]:
    path = os.fspath(path)
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state dict (a mapping of names to tensors)")
    if "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    return {k: v for k, v in sd.items() if isinstance(v, Tensor)}


class LpipsWeights:
    """AlexNet's five convolutions and the five ``lin`` vectors, unpacked (``conv_w``, ``conv_b``, ``lin``: the tests'
    view) and packed once into the kernel's layout (``packed_w``).  All float32 on ``device``."""

    def __init__(self, conv_w: Sequence[Tensor], conv_b: Sequence[Tensor], lin: Sequence[Tensor], device="cpu"):
        device = torch.device(device)
        self.device = device
        self.conv_w, self.conv_b, self.lin = [], [], []
        for l, (cin, cout, k, _, _) in enumerate(LAYERS):
            w, b, v = conv_w[l], conv_b[l], lin[l]
            _check_shape(f"features.{FEATURE_KEYS[l]}.weight", w, (cout, cin, k, k))
            _check_shape(f"features.{FEATURE_KEYS[l]}.bias", b, (cout,))
            if v.numel() != cout:
                raise ValueError(f"lin{l}.model.1.weight: shape {tuple(v.shape)}, expected (1, {cout}, 1, 1)")
            self.conv_w.append(w.detach().to(device=device, dtype=torch.float32).contiguous())
            self.conv_b.append(b.detach().to(device=device, dtype=torch.float32).contiguous())
            self.lin.append(v.detach().to(device=device, dtype=torch.float32).reshape(cout).contiguous())
        self.device = self.conv_w[0].device                  # ("cuda" has become "cuda:0")
        self.packed_w = [pack_conv(w, l) for l, w in enumerate(self.conv_w)]

    @classmethod
    def load(cls, path_or_paths, device="cpu") -> "LpipsWeights":
        """One merged file or a pair of files (.pth / .pt state dicts, read with ``weights_only=True``, or .npz) holding
        torchvision's AlexNet keys ``features.{0,3,6,8,10}.{weight,bias}`` and the ``lpips`` package's linear layers
        ``lin{0..4}.model.1.weight`` ([1,C,1,1]).  A missing key or a wrong shape raises ``ValueError`` naming the key.
        Nothing is ever fetched."""
        if isinstance(path_or_paths, (str, os.PathLike)):
            s = os.fspath(path_or_paths)
            paths = s.split(os.pathsep) if os.pathsep in s else [s]
        else:
            paths = [os.fspath(p) for p in path_or_paths]
        sd: Dict[str, Tensor] = {}
        for p in paths:
            sd.update(_read(p))

        def get(key: str, shape) -> Tensor:
            if key not in sd:
                raise ValueError(f"LPIPS weights: key '{key}' is missing from {', '.join(paths)}")
            _check_shape(key, sd[key], shape)
            return sd[key]

        conv_w, conv_b, lin = [], [], []
        for l, (cin, cout, k, _, _) in enumerate(LAYERS):
            i = FEATURE_KEYS[l]
            conv_w.append(get(f"features.{i}.weight", (cout, cin, k, k)))
            conv_b.append(get(f"features.{i}.bias", (cout,)))
            lin.append(get(f"lin{l}.model.1.weight", (1, cout, 1, 1)))
        return cls(conv_w, conv_b, lin, device)

    def to(self, device) -> "LpipsWeights":
        device = torch.device(device)
        if device == self.device or (device.type == self.device.type and device.index is None):
            return self
        return LpipsWeights(self.conv_w, self.conv_b, self.lin, device)

    def state_dict(self) -> Dict[str, Tensor]:
        """The merged file's keys (what ``load`` reads back)."""
        sd = {}
        for l, i in enumerate(FEATURE_KEYS):
            sd[f"features.{i}.weight"] = self.conv_w[l]
            sd[f"features.{i}.bias"] = self.conv_b[l]
            sd[f"lin{l}.model.1.weight"] = self.lin[l].reshape(1, -1, 1, 1)
        return sd


def _check_shape(key: str, t: Tensor, shape) -> None:
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"LPIPS weights: key '{key}' has shape {tuple(t.shape)}, expected {tuple(shape)}")


def resolve_weights(spec: Union[None, str, os.PathLike, Sequence, LpipsWeights], device) -> Optional[LpipsWeights]:
    """None / a path (or two, as a sequence or joined by ``os.pathsep``) / a LpipsWeights -> LpipsWeights on ``device``."""
    if spec is None:
        return None
    if isinstance(spec, LpipsWeights):
        return spec.to(device)
    return LpipsWeights.load(spec, device)


# ---- workspaces: feature maps and partial sums, one set per (device, stream, H, W) --------------------------------------
# About 200 MB at 1080p.  Keyed by the stream too, so that two streams working at one size never share buffers; the least
# recently used sets beyond WORKSPACE_SETS are dropped, so an evaluation set of many image sizes does not pile them up (a
# training loop and its eval images keep theirs).
WORKSPACE_SETS = 4
_WORK: "collections.OrderedDict[Tuple[torch.device, int, int, int], dict]" = collections.OrderedDict()


def _workspace(device: torch.device, stream: int, H: int, W: int) -> dict:
    key = (device, stream, H, W)
    ws = _WORK.get(key)
    if ws is not None:
        _WORK.move_to_end(key)
        return ws
    sizes = feature_sizes(H, W)
    feats = [torch.empty(2, h, w, LAYERS[l][1], dtype=torch.float32, device=device) for l, (h, w) in enumerate(sizes)]
    pools = {l: torch.empty(2, sizes[l][0], sizes[l][1], LAYERS[l][0], dtype=torch.float32, device=device)
             for l in POOL_BEFORE}
    ws = _WORK[key] = {"sizes": sizes, "feats": feats, "pools": pools,
                       "partials": torch.empty(L.LPIPS_WS_DOUBLES, dtype=torch.float64, device=device)}
    while len(_WORK) > WORKSPACE_SETS:
        _WORK.popitem(last=False)       # (the allocator keeps a dropped set's memory alive until the stream has passed it)
    return ws


def _image(img: Tensor) -> Tensor:
    """[1,3,H,W] / [3,H,W] / [H,W,3], float or uint8 (divided by 255) -> contiguous float32 [H,W,3]."""
    from .metrics import _to_hwc
    if img.dim() not in (3, 4) or (img.dim() == 4 and img.shape[0] != 1):
        raise ValueError(f"an image must be [H,W,3], [3,H,W] or [1,3,H,W], got {tuple(img.shape)}")
    img = _to_hwc(img)
    if img.dim() != 3 or img.shape[-1] != 3:
        raise ValueError(f"an image must have 3 channels, got {tuple(img.shape)}")
    return img.to(torch.float32).contiguous()


@torch.no_grad()
def lpips(pred: Tensor, gt: Tensor, weights: LpipsWeights, *, return_features: bool = False, return_layers: bool = False):
    """LPIPS (AlexNet) of two images as a 0-dim float32 device tensor.  Images: [H,W,3], [3,H,W] or [1,3,H,W], values
    in [0, 1] (uint8 is divided by 255).  torchmetrics' range check on the input needs a host read and is not
    reproduced: values outside [0, 1] are taken as they are.  H or W below 31 raises ``ValueError``.

    Feature maps and partial sums come from a cached workspace (per device, stream and size).  What a call still takes
    from torch's caching allocator: the six result floats (the returned value is a view of them, so it stays valid when
    the next call runs) and, only for input that is not already contiguous float32 [H,W,3], the converted copies.

    ``return_features``: also the five post-ReLU feature maps, each [2,C,h,w] (copies; image 0 = ``pred``).
    ``return_layers``: also the five per-layer terms, float32[5] (they sum to the value)."""
    p, g = _image(pred), _image(gt)
    if p.shape != g.shape:
        raise ValueError(f"the images differ in shape: {tuple(p.shape)} and {tuple(g.shape)}")
    H, W, _ = p.shape
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError(f"LPIPS needs images of at least {MIN_SIDE} x {MIN_SIDE} pixels, got {H} x {W}")
    if not p.is_cuda:
        raise L.QedSplatError("lpips: the images must be on the GPU (there is no CPU path)")
    g = g.to(p.device)
    if weights.device != p.device:
        raise ValueError(f"the weights are on {weights.device}, the images on {p.device}: use weights.to(device)")
    lib = L.load()
    st = L.current_stream()
    ws = _workspace(p.device, st, H, W)
    in0, in1, h, w = p, g, H, W
    for l in range(5):
        if l in POOL_BEFORE:
            pooled = ws["pools"][l]
            L.check(lib.qed_lpips_pool(LAYERS[l][0], h, w, L.ptr(ws["feats"][l - 1]), L.ptr(pooled), st), "qed_lpips_pool")
            h, w = pooled.shape[1], pooled.shape[2]
            in0, in1 = pooled[0], pooled[1]
        out = ws["feats"][l]
        L.check(lib.qed_lpips_conv(l, h, w, L.ptr(in0), L.ptr(in1), L.ptr(weights.packed_w[l]), L.ptr(weights.conv_b[l]),
                                   L.ptr(out), st), "qed_lpips_conv")
        h, w = out.shape[1], out.shape[2]
        in0, in1 = out[0], out[1]
        L.check(lib.qed_lpips_distance(l, h, w, L.ptr(out), L.ptr(weights.lin[l]), L.ptr(ws["partials"]), st),
                "qed_lpips_distance")
    res = torch.empty(6, dtype=torch.float32, device=p.device)
    L.check(lib.qed_lpips_finalize(*[a * b for a, b in ws["sizes"]], L.ptr(ws["partials"]), L.ptr(res), st),
            "qed_lpips_finalize")
    value = res[0]
    if not (return_features or return_layers):
        return value
    ret = [value]
    if return_features:
        ret.append([f.permute(0, 3, 1, 2).contiguous() for f in ws["feats"]])
    if return_layers:
        ret.append(res[1:])
    return tuple(ret)


def main(argv=None) -> None:
    from PIL import Image
    ap = argparse.ArgumentParser(prog="python -m qed_splatter_amd.lpips",
                                 description="LPIPS (AlexNet) between two images, from user-supplied weights")
    ap.add_argument("--pred", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--weights", required=True, nargs="+", help="one merged file, or AlexNet's and the lin layers' files")
    args = ap.parse_args(argv)
    if len(args.weights) > 2:
        ap.error("--weights takes one merged file or a pair of files")
    dev = torch.device("cuda:0")
    weights = LpipsWeights.load(args.weights, dev)
    imgs = [torch.from_numpy(np.asarray(Image.open(f).convert("RGB"))).to(dev) for f in (args.pred, args.gt)]
    value, layers = lpips(imgs[0], imgs[1], weights, return_layers=True)
    print(json.dumps({"lpips": float(value), "layers": [float(x) for x in layers], "height": int(imgs[0].shape[0]),
                      "width": int(imgs[0].shape[1])}))


if __name__ == "__main__":
    main()
