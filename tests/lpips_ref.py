"""Plain-torch restatement of the LPIPS (AlexNet) formulas of qed_splatter_amd/lpips.py, in float64 (the tests'
reference) or float32 (to show that the tests' bound is attainable in float32 at all), with a seeded weight generator:
no pretrained weights exist where the tests run, and the arithmetic does not care."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

EPS = 1e-8
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
FEATURE_KEYS = (0, 3, 6, 8, 10)


def make_state_dict(seed: int = 0) -> dict:
    """Merged state dict (torchvision's AlexNet keys + the lpips package's lin keys), float32 on the CPU: convolution
    weights uniform in +-sqrt(6 / fan_in), biases in +-0.1, lin weights in [0, 0.2)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for l, (cin, cout, k, _, _) in enumerate(LAYERS):
        bound = math.sqrt(6.0 / (cin * k * k))
        sd[f"features.{FEATURE_KEYS[l]}.weight"] = (torch.rand(cout, cin, k, k, generator=g) * 2 - 1) * bound
        sd[f"features.{FEATURE_KEYS[l]}.bias"] = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
        sd[f"lin{l}.model.1.weight"] = torch.rand(1, cout, 1, 1, generator=g) * 0.2
    return sd


def make_images(H: int, W: int, seed: int = 0):
    """[H,W,3] float32 pair: uniform a, b = clamp(a + 0.1 noise, 0, 1)."""
    g = torch.Generator().manual_seed(1000 + seed)
    a = torch.rand(H, W, 3, generator=g)
    b = (a + 0.1 * torch.randn(H, W, 3, generator=g)).clamp(0.0, 1.0)
    return a, b


def reference(a_hwc: torch.Tensor, b_hwc: torch.Tensor, sd: dict, dtype=torch.float64):
    """(value, the five per-layer terms [5], the five post-ReLU feature maps [2,C,h,w]) in ``dtype`` on the CPU."""
    x = torch.stack([a_hwc, b_hwc]).cpu().to(dtype).permute(0, 3, 1, 2)
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    x = (x - shift) / scale                                   # before conv1's zero padding
    feats, terms = [], []
    for l, (_, _, _, stride, pad) in enumerate(LAYERS):
        if l in (1, 2):
            x = F.max_pool2d(x, kernel_size=3, stride=2)      # no padding, floor
        w = sd[f"features.{FEATURE_KEYS[l]}.weight"].to(dtype)
        b = sd[f"features.{FEATURE_KEYS[l]}.bias"].to(dtype)
        x = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
        feats.append(x)
        n = x / torch.sqrt(EPS + (x * x).sum(dim=1, keepdim=True))
        lin = sd[f"lin{l}.model.1.weight"].to(dtype).view(1, -1, 1, 1)
        d = (lin * (n[0:1] - n[1:2]) ** 2).sum(dim=1)         # [1,h,w]
        terms.append(d.mean())
    terms = torch.stack(terms)
    return terms.sum(), terms, feats
