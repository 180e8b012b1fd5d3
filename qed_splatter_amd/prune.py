"""Prune Gaussians by their blending contribution over a set of views.

    python -m qed_splatter_amd.prune --load CKPT --data DIR --output CKPT2
        [--score max|sum --min-score X | --keep-fraction F] [--volume-power B] [--stride S]
        [--split train|all] [--export-ply PLY] [--eval]

Every other route that changes the number of Gaussians judges them by proxies (opacity, scale, screen size, the
positional gradient).  This one measures what a Gaussian does to the pictures: its blending weight ``w = alpha * T``
at every pixel of every scored view, reduced per Gaussian to the maximum, the sum and the number of pixels it
contributes to (``qed_contribution``, csrc/importance.hip: the compositing forward's walk over the lists the render
already made -- no second projection, no second binning).

The two selection rules are RESTATED FROM MEMORY of the papers, not checked against their code:
  * ``score="max"``: keep ``max_weight >= min_score`` (RadSplat; its threshold 0.01 is the default);
  * ``score="sum"``: ``sum_weight * (prod exp(scales) / its 0.9 quantile, clamped to 1) ** volume_power``
    (LightGaussian's volume term), usually with ``keep_fraction``.

The Gaussian that TERMINATES a pixel is not applied by the renderer (gsplat's rule), so it scores zero there; one that
only ever terminates pixels is pruned, the walk then continues past it and those pixels can change by up to the
transmittance that was left (at most 0.1 when the terminator's alpha is 0.999).  Documented, not fixed.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import time
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch
from torch import Tensor

from . import _lib as L

FIXED_ONE = 4294967296.0        # sum_weight: unsigned 64-bit fixed point, 32 fractional bits
_stream = L.current_stream


class ContributionScores:
    """The three [N] score buffers of ``qed_contribution``; they accumulate over ``add_view`` calls.

    ``max_weight`` is kept as the bit pattern of a non-negative float in 32 bits (an integer max is the float max),
    ``sum_weight`` as unsigned 64-bit fixed point with 32 fractional bits (capacity 2^32 units of weight per Gaussian:
    every pixel of 2 000 views at 1920x1080 at alpha 0.999; not guarded), ``hits`` as 32 bits.  All three are updated
    with order-independent integer operations: the same bits for any order of views."""

    def __init__(self, n: int, device):
        self.n, self.device = int(n), torch.device(device)
        self._max = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self._sum = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        self._hits = torch.zeros(self.n, dtype=torch.int32, device=self.device)

    def zero_(self) -> "ContributionScores":
        self._max.zero_(); self._sum.zero_(); self._hits.zero_()
        return self

    def max_weight(self) -> Tensor:
        """[N] float32: a view of the buffer."""
        return self._max.view(torch.float32)

    def sum_weight(self) -> Tensor:
        """[N] float64."""
        hi = (self._sum >> 32) & 0xFFFFFFFF          # (the buffer is unsigned: bit 63 is a value bit)
        lo = self._sum & 0xFFFFFFFF
        return hi.to(torch.float64) + lo.to(torch.float64) / FIXED_ONE

    def hits(self) -> Tensor:
        """[N] int64."""
        return self._hits.to(torch.int64) & 0xFFFFFFFF

    def raw(self):
        """The three buffers as stored (bit-for-bit comparisons)."""
        return self._max, self._sum, self._hits

    def add_view(self, info: Dict, C_: int, N: int, width: int, height: int, pixel_mask: Optional[Tensor] = None,
                 launch_flags: Optional[int] = None) -> None:
        """Score the ``C_`` views of one ``rasterization(..., _keep_records=True)`` / ``get_outputs`` ``info``: one kernel
        call on the records and tile lists that call left.  ``pixel_mask`` [C,H,W] (or [H,W(,1)] for one view), any dtype:
        a pixel whose entry is 0 votes in none of the scores."""
        if N != self.n:
            raise ValueError(f"add_view: the scores hold {self.n} Gaussians, the view has {N}")
        ids = info["flatten_ids"]
        mask = None
        if pixel_mask is not None:
            mask = (pixel_mask.reshape(C_, height, width) != 0).to(device=self.device, dtype=torch.uint8).contiguous()
        if self.device.type != "cuda":
            _add_view_torch(self, info, C_, N, width, height, mask)
            return
        splats, offsets = info["_splats"], info["_isect_offsets_full"]
        tw, th = int(info["tile_width"]), int(info["tile_height"])
        flags = L.composite_launch_flags() if launch_flags is None else int(launch_flags)
        L.check(L.load().qed_contribution(C_, N, L.ptr(splats), L.ptr(ids) if ids is not None and ids.numel() else None,
                                          L.ptr(offsets), int(width), int(height), tw, th, L.ptr(mask), L.ptr(self._max),
                                          L.ptr(self._sum), L.ptr(self._hits), flags, _stream()), "qed_contribution")


def _add_view_torch(scores: ContributionScores, info: Dict, C_: int, N: int, width: int, height: int,
                    mask: Optional[Tensor]) -> None:
    """The torch body of ``add_view`` for an ``info`` on the CPU (the oracle's, or a GPU one moved over): a plain loop over
    the tiles in float64.  Not a reference for anything: the tests have their own."""
    if "_splats" in info:
        rec = info["_splats"].reshape(C_ * N, -1).double()
        xy, con, op = rec[:, 0:2], rec[:, 2:5], rec[:, 5]
    else:
        xy = info["means2d"].detach().reshape(C_ * N, 2).double()
        con = info["conics"].detach().reshape(C_ * N, 3).double()
        op = info["opacities"].detach().reshape(C_ * N).double()
    ids = info["flatten_ids"].to(torch.int64)
    tw, th = int(info["tile_width"]), int(info["tile_height"])
    offs = info["_isect_offsets_full"] if "_isect_offsets_full" in info else info["isect_offsets"]
    offs = offs.reshape(-1).to(torch.int64).tolist()
    offs = offs[: C_ * tw * th] + [ids.numel()]
    wmax = scores.max_weight()
    for t in range(C_ * tw * th):
        s, e = offs[t], offs[t + 1]
        if e <= s:
            continue
        cam, ty, tx = t // (tw * th), (t % (tw * th)) // tw, t % tw
        py, px = torch.meshgrid(torch.arange(ty * 16, min(ty * 16 + 16, height)),
                                torch.arange(tx * 16, min(tx * 16 + 16, width)), indexing="ij")
        py, px = py.reshape(-1), px.reshape(-1)
        if mask is not None:
            live = mask[cam, py, px] != 0
            py, px = py[live], px[live]
        if py.numel() == 0:
            continue
        g = ids[s:e]
        dx = xy[g, 0][None, :] - (px.double()[:, None] + 0.5)
        dy = xy[g, 1][None, :] - (py.double()[:, None] + 0.5)
        sigma = 0.5 * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) + con[g, 1] * dx * dy
        a = torch.clamp(op[g][None, :] * torch.exp(-sigma), max=0.999)
        a = torch.where((sigma >= 0) & (a >= 1.0 / 255.0), a, torch.zeros_like(a))
        t_after = torch.cumprod(1.0 - a, dim=1)
        t_before = torch.cat([torch.ones_like(t_after[:, :1]), t_after[:, :-1]], dim=1)
        w = torch.where((a > 0) & (t_after > 1e-4), a * t_before, torch.zeros_like(a))
        rows = g - cam * N
        wmax[rows] = torch.maximum(wmax[rows], w.amax(dim=0).float())        # (a Gaussian is listed once per tile)
        scores._sum.index_add_(0, rows, torch.round(w.sum(dim=0).float().double() * FIXED_ONE).to(torch.int64))
        scores._hits.index_add_(0, rows, (w > 0).sum(dim=0).to(torch.int32))


@torch.no_grad()
def score_views(model, cameras: Sequence, masks: Optional[Sequence] = None, stride: int = 1,
                scores: Optional[ContributionScores] = None) -> ContributionScores:
    """Render every ``stride``-th camera in evaluation mode at full resolution, with the model's current SH degree and
    rasterize mode, and score it.  The crop box is not applied (a pruned model is a model, not a view of one).
    ``masks``: per camera a [H,W(,1)] mask or None."""
    if scores is None:
        scores = ContributionScores(model.num_points, model.device)
    was_training, crop_box, normals = model.training, model.crop_box, getattr(model.config, "output_normals", False)
    model.eval()
    model.crop_box = None
    model.config.output_normals = False
    model.__dict__["_score_records"] = True
    try:
        for k in range(0, len(cameras), max(int(stride), 1)):
            out = model.get_outputs(cameras[k])
            h, w = int(out["rgb"].shape[-3]), int(out["rgb"].shape[-2])
            info = model.info
            mask = masks[k] if masks is not None else None
            scores.add_view(info, int(info["n_cameras"]), model.num_points, w, h, mask)
            info.pop("_splats", None)
            info.pop("_isect_offsets_full", None)
    finally:
        model.__dict__.pop("_score_records", None)
        model.config.output_normals = normals
        model.crop_box = crop_box
        model.train(was_training)
    return scores


@dataclass
class PruneConfig:
    """``score`` "max" (RadSplat's rule) or "sum" (LightGaussian's, with ``volume_power``); rows whose selection score is
    below ``min_score`` go; with ``keep_fraction`` the best ``ceil(f N)`` rows stay instead (ties by row index)."""
    score: str = "max"
    min_score: float = 0.01
    keep_fraction: Optional[float] = None
    volume_power: float = 0.0


def selection_score(config: PruneConfig, max_weight: Tensor, sum_weight: Tensor, scales: Optional[Tensor] = None) -> Tensor:
    """[N] float64.  ``scales``: the model's log-scales [N,3] (only read with ``volume_power`` != 0)."""
    if config.score == "max":
        return max_weight.to(torch.float64)
    if config.score != "sum":
        raise ValueError(f"PruneConfig.score must be 'max' or 'sum', not {config.score!r}")
    s = sum_weight.to(torch.float64)
    if config.volume_power != 0.0 and s.numel():
        vol = torch.exp(scales.detach().to(torch.float64).sum(dim=-1))            # prod exp(scales)
        v90 = torch.quantile(vol, 0.9)
        s = s * torch.clamp(vol / v90, max=1.0) ** float(config.volume_power)
    return s


def selection_threshold(config: PruneConfig, score: Tensor):
    """``(min_score, tie_below)``: row i stays when score[i] > min_score, or score[i] == min_score and i < tie_below."""
    n = score.numel()
    if config.keep_fraction is None:
        return float(config.min_score), n
    f = float(config.keep_fraction)
    if not 0.0 <= f <= 1.0:
        raise ValueError("PruneConfig.keep_fraction must be in [0, 1]")
    k = min(int(math.ceil(f * n)), n)
    if k == 0:
        return float("inf"), 0
    thr = torch.kthvalue(score, n - k + 1).values                               # the k-th largest
    above = int((score > thr).sum())
    ties = torch.nonzero(score == thr).reshape(-1)
    return float(thr), int(ties[k - above - 1]) + 1


def keep_mask(config: PruneConfig, max_weight: Tensor, sum_weight: Tensor, scales: Optional[Tensor] = None) -> Tensor:
    """[N] bool: the rows a prune with ``config`` keeps (the torch statement of what qed_prune_classify decides)."""
    score = selection_score(config, max_weight, sum_weight, scales)
    thr, tie_below = selection_threshold(config, score)
    idx = torch.arange(score.numel(), device=score.device)
    return (score > thr) | ((score == thr) & (idx < tie_below))


@torch.no_grad()
def prune(model, optimizer, scores: ContributionScores, config: Optional[PruneConfig] = None, densifier=None,
          captured_step=None, field=None) -> Dict:
    """Drop the low scorers from ``model`` and both Adam moments of ``optimizer`` (a FlatAdam; None: parameters only).
    Survivors keep their order and their bits.  Returns ``n_before``, ``n_after``, ``n_pruned``, ``threshold``.
    ``densifier``: its running statistics (length N) are cleared.  ``field`` (a semantic.SemanticField of the model's N): the
    result also holds ``"field"``, the field of the pruned model (``field.select`` of the keep mask: the survivors' rows
    and moments, bit for bit).

    Refused: ``strategy="mcmc"`` (relocation owns dead Gaussians there and the count is a target), and a
    ``captured_step`` (graph.GraphedTrainStep): it replays launches on the buffers of the old N and ``rebind_flat`` cannot
    reach it -- prune, then capture again.  (The captured segments of get_outputs are keyed on N and the parameters'
    addresses, so ``rebind_flat`` retires them by itself.)"""
    config = config or PruneConfig()
    if getattr(model.config, "strategy", "default") == "mcmc":
        raise NotImplementedError("prune: strategy='mcmc' keeps a fixed budget and relocates its dead Gaussians itself")
    if captured_step is not None:
        raise NotImplementedError("prune: a captured training step holds launches on the buffers of the old N; prune "
                                  "first and capture (or recapture()) afterwards")
    n, dev = model.num_points, model.device
    if scores.n != n:
        raise ValueError(f"prune: the scores hold {scores.n} Gaussians, the model has {n}")
    if field is not None:
        field.check_model(model)
    score = selection_score(config, scores.max_weight(), scores.sum_weight(), model.scales)
    thr, tie_below = selection_threshold(config, score)
    info = {"n_before": n, "n_after": n, "n_pruned": 0, "threshold": thr}
    if n == 0:
        if field is not None:
            info["field"] = field
        return info
    old_m = optimizer.exp_avg if optimizer is not None else None
    old_v = optimizer.exp_avg_sq if optimizer is not None else None
    if dev.type == "cuda":
        lib = L.load()
        flags = torch.empty(n, dtype=torch.uint8, device=dev)
        pos = torch.empty(lib.qed_densify_pos_ints(n), dtype=torch.int32, device=dev)
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        score = score.contiguous()
        L.check(lib.qed_prune_classify(n, L.ptr(score), thr, tie_below, L.ptr(flags), L.ptr(pos), L.ptr(totals), _stream()),
                "qed_prune_classify")
        k = int(totals[1])                                                      # the one host sync of a prune
        new = model.layout.resized(k)
        new_p, new_m, new_v = new.empty_like_state(dev)
        if optimizer is None:                                                   # (the emit pass copies three buffers)
            old_m = old_v = model.flat_params
        h_tot = (C.c_int32 * 4)(0, k, 0, 0)
        L.check(lib.qed_densify_emit(n, 1, L.ptr(flags), L.ptr(pos), C.cast(h_tot, C.c_void_p), None,
                                     L.ptr(model.flat_params), L.ptr(old_m), L.ptr(old_v), model.layout.c_begin_ptr,
                                     L.ptr(new_p), L.ptr(new_m), L.ptr(new_v), new.c_begin_ptr, _stream()),
                "qed_densify_emit")
        kept = flags != 0
    else:
        idx = torch.arange(n, device=dev)
        keep = torch.nonzero((score > thr) | ((score == thr) & (idx < tie_below))).reshape(-1)
        k = int(keep.numel())
        kept = torch.zeros(n, dtype=torch.bool, device=dev)
        kept[keep] = True
        new = model.layout.resized(k)
        new_p, new_m, new_v = new.empty_like_state(dev)
        for src, dst in ((model.flat_params, new_p), (old_m, new_m), (old_v, new_v)):
            if src is None:
                continue
            for (name, a), b in zip(model.layout.views(src).items(), new.views(dst).values()):
                b.copy_(a.detach()[keep])
    model.rebind_flat(new_p, k)
    if optimizer is not None:
        optimizer.rebind(new_m, new_v)
    if densifier is not None:
        densifier.xys_grad_norm = densifier.vis_counts = densifier.max_2Dsize = None
    info.update(n_after=k, n_pruned=n - k)
    if field is not None:
        info["field"] = field.select(kept)
    return info


def main(argv=None) -> Dict:
    from .render import add_dataparser_arguments, dataset_path, load_model
    ap = argparse.ArgumentParser(prog="python -m qed_splatter_amd.prune", description="Prune Gaussians by their blending contribution over the dataset's views")
    ap.add_argument("--load", required=True, metavar="CKPT", help="a checkpoint written by train.py --save")
    ap.add_argument("--data", required=True, metavar="DIR", help="the dataset of the training run")
    ap.add_argument("--output", required=True, metavar="CKPT2")
    ap.add_argument("--score", choices=("max", "sum"), default="max")
    ap.add_argument("--min-score", type=float, default=None, help="default 0.01 with --score max")
    ap.add_argument("--keep-fraction", type=float, default=None)
    ap.add_argument("--volume-power", type=float, default=0.0)
    ap.add_argument("--stride", type=int, default=1, help="score every S-th view")
    ap.add_argument("--split", choices=("train", "all"), default="train")
    ap.add_argument("--export-ply", metavar="PLY", default=None)
    ap.add_argument("--eval", action="store_true", help="Trainer.evaluate_images before and after")
    ap.add_argument("--background-color", choices=("random", "black", "white"), default="random")
    add_dataparser_arguments(ap)
    a = ap.parse_args(argv)
    if a.min_score is not None and a.keep_fraction is not None:
        ap.error("--min-score and --keep-fraction: give one")
    if a.min_score is None and a.keep_fraction is None and a.score != "max":
        ap.error("--score sum needs --min-score or --keep-fraction")
    if not torch.cuda.is_available():
        raise SystemExit("qed_splatter_amd.prune needs a GPU")
    from .datamanager import FullImageDatamanager
    from .dataparser import DataparserConfig
    from .model import FlatAdam
    from .train import evaluate_image_items
    L.load()
    device = torch.device("cuda:0")
    model, ckpt = load_model(a.load, device, a.background_color)
    optimizer = FlatAdam(model, means_schedule=FlatAdam.MEANS_SCHEDULE)
    if "optimizer" in ckpt:
        optimizer.load_state_dict(ckpt["optimizer"])
    dp_cfg = DataparserConfig(orientation_method=a.orientation_method, center_method=a.center_method,
                              auto_scale_poses=a.auto_scale_poses == "True", depth_unit_scale_factor=a.depth_unit_scale_factor,
                              train_split_fraction=a.train_split_fraction, scale_factor=a.scale_factor, undistort=a.undistort)
    dm = FullImageDatamanager(a.data, dp_cfg, device=a.cache_device)
    items = list(dm.train_items() if a.split == "train" else dm.all_items())
    cameras = [cam for cam, _ in items]
    masks = [b["mask"] if "mask" in b else None for _, b in items]
    result: Dict = {"views": len(range(0, len(cameras), max(a.stride, 1)))}
    if a.eval:
        result["eval_before"] = evaluate_image_items(model, dm.eval_items())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores = score_views(model, cameras, masks if any(m is not None for m in masks) else None, a.stride)
    torch.cuda.synchronize()
    result["score_seconds"] = time.perf_counter() - t0
    config = PruneConfig(score=a.score, min_score=0.01 if a.min_score is None else a.min_score,
                         keep_fraction=a.keep_fraction, volume_power=a.volume_power)
    result.update(prune(model, optimizer, scores, config))
    if a.eval:
        result["eval_after"] = evaluate_image_items(model, dm.eval_items())
    from .layout import GROUP_ORDER
    out = dict(ckpt)
    out["params"] = {n: model.gauss_params[n].detach().clone() for n in GROUP_ORDER}
    out["optimizer"] = optimizer.state_dict()
    torch.save(out, a.output)
    if a.export_ply:
        from .gaussian_ply import export_gaussian_ply
        res = export_gaussian_ply(model, a.export_ply, frame="model",
                                  dataparser_transform=ckpt.get("dataparser_transform"),
                                  dataparser_scale=ckpt.get("dataparser_scale", 1.0))
        result["exported"] = int(res["written"])
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
