"""Semantic label fields on a trained model.

    python -m qed_splatter_amd.semantic fit  --load CKPT --data DIR --output FIELD.pt [--steps N --lr X --classes-file JSON --stride S]
    python -m qed_splatter_amd.semantic eval --load CKPT --field FIELD.pt --data DIR [--split eval] --output-path OUT.json

The datasets the reference is used on carry per-image class maps (terrain, obstacle, sky, person) next to their depth
frames (``label_path`` of a frame: an 8-bit single-channel PNG, value = class, 255 = unlabelled; dataparser.py).  A
``SemanticField`` gives every Gaussian of a trained model a row of class logits; the logits of a pixel are the rows
composited with the render's own blending weights ``w_i = alpha_i T_i`` (LangSplat's / Feature-3DGS's route, restated from
memory of the papers).  The geometry is FROZEN: no gradient reaches means, scales, quaternions, opacities or SH, the colour
pass is never differentiated, and nothing here goes through torch autograd.

The kernels (csrc/semantic.hip; include/qed_splat.h has their contract): ``qed_features_fwd`` / ``qed_features_bwd`` walk the
records and tile lists an evaluation render left behind (``rasterization(..., _keep_records=True)``, as prune.score_views
does: no second projection, no second binning) and take the render's accept / skip / terminate decisions; ``qed_label_loss``
is the weighted softmax cross-entropy with its gradient, ``qed_label_confusion`` the confusion counts, ``qed_label_present``
the planes render.py writes.  ``qed_adam_step`` steps the table.

Not offered: gradients to the geometry, more than 32 channels or continuous feature distillation, labels on
undistorted datasets, labels in surface_cloud.py, the data-parallel exchange.
"""
from __future__ import annotations

import argparse
import colorsys
import ctypes as C
import json
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib as L

MAX_CLASSES = L.FEATURES_MAX
_stream = L.current_stream


def default_palette(n_classes: int) -> Tensor:
    """[K + 1, 3] uint8: K hues a golden-ratio step apart at two brightness levels, and black for "no prediction"."""
    rows = []
    for k in range(n_classes):
        r, g, b = colorsys.hsv_to_rgb((0.11 + 0.618033988749895 * k) % 1.0, 0.75, 0.95 if k % 2 == 0 else 0.7)
        rows.append([int(round(255 * r)), int(round(255 * g)), int(round(255 * b))])
    rows.append([0, 0, 0])
    return torch.tensor(rows, dtype=torch.uint8)


class SemanticField:
    """The [N,K] float32 table of class logits of a model's N Gaussians (zeros: every class equally likely), both Adam
    moments, the step count, the class names and the [K + 1, 3] uint8 palette (its last row colours pixels without a
    prediction)."""

    def __init__(self, n_gaussians: int, n_classes: int, device="cpu", class_names: Optional[Sequence[str]] = None,
                 palette: Optional[Tensor] = None):
        n, k = int(n_gaussians), int(n_classes)
        if not 1 <= k <= MAX_CLASSES:
            raise ValueError(f"SemanticField: {k} classes; 1..{MAX_CLASSES} are offered")
        if n < 0:
            raise ValueError("SemanticField: a negative number of Gaussians")
        self.device = torch.device(device)
        self.logits = torch.zeros(n, k, dtype=torch.float32, device=self.device)
        self.exp_avg = torch.zeros_like(self.logits)
        self.exp_avg_sq = torch.zeros_like(self.logits)
        self.step = 0
        self.class_names = [str(s) for s in class_names] if class_names is not None else [f"class_{i}" for i in range(k)]
        if len(self.class_names) != k:
            raise ValueError(f"SemanticField: {len(self.class_names)} class names for {k} classes")
        pal = default_palette(k) if palette is None else torch.as_tensor(palette)
        if tuple(pal.shape) != (k + 1, 3) or pal.dtype != torch.uint8:
            raise ValueError(f"SemanticField: the palette is a [{k + 1}, 3] uint8 table (its last row: no prediction)")
        self.palette = pal.to(self.device).contiguous()

    @property
    def n_gaussians(self) -> int:
        return int(self.logits.shape[0])

    @property
    def n_classes(self) -> int:
        return int(self.logits.shape[1])

    def check_model(self, model) -> None:
        if model.num_points != self.n_gaussians:
            raise ValueError(f"the field holds {self.n_gaussians} Gaussians, the model has {model.num_points}")

    def state_dict(self) -> Dict:
        return {"logits": self.logits.detach().clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "step": int(self.step), "class_names": list(self.class_names), "palette": self.palette.clone()}

    def load_state_dict(self, state: Dict) -> "SemanticField":
        if tuple(state["logits"].shape) != tuple(self.logits.shape):
            raise ValueError(f"load_state_dict: the state is {tuple(state['logits'].shape)}, the field "
                             f"{tuple(self.logits.shape)}")
        for name in ("logits", "exp_avg", "exp_avg_sq"):
            getattr(self, name).copy_(state[name].to(self.device, torch.float32))
        self.step = int(state["step"])
        self.class_names = [str(s) for s in state["class_names"]]
        self.palette = state["palette"].to(self.device, torch.uint8).contiguous()
        return self

    @classmethod
    def from_state_dict(cls, state: Dict, device="cpu") -> "SemanticField":
        n, k = state["logits"].shape
        return cls(n, k, device, state["class_names"], state["palette"].cpu()).load_state_dict(state)

    def save(self, path) -> None:
        torch.save({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, device="cpu") -> "SemanticField":
        return cls.from_state_dict(torch.load(path, map_location="cpu", weights_only=True), device)

    def select(self, keep_mask: Tensor) -> "SemanticField":
        """The field of a pruned model: the rows (and moments) where ``keep_mask`` [N] is set, in order, bit for bit."""
        keep = keep_mask.reshape(-1).to(self.device) != 0
        if keep.numel() != self.n_gaussians:
            raise ValueError(f"select: a mask of {keep.numel()} for {self.n_gaussians} Gaussians")
        out = SemanticField(int(keep.sum()), self.n_classes, self.device, self.class_names, self.palette.cpu())
        out.logits, out.exp_avg, out.exp_avg_sq = (t[keep].contiguous() for t in (self.logits, self.exp_avg, self.exp_avg_sq))
        out.step = self.step
        return out


def gaussian_labels(field: SemanticField) -> Tensor:
    """[N] uint8: the class of every Gaussian (the first maximum of its row)."""
    if field.n_gaussians == 0:
        return torch.empty(0, dtype=torch.uint8, device=field.device)
    return field.logits.argmax(dim=1).to(torch.uint8)


# ---- the kernels on one render's records ---------------------------------------------------------------------------------
def _lists(info: Dict, who: str):
    if "_splats" not in info or "_isect_offsets_full" not in info:
        raise ValueError(f"{who} needs the records of the colour pass: rasterization(..., _keep_records=True)")
    ids = info["flatten_ids"]
    return (info["_splats"], ids if ids is not None and ids.numel() else None, info["_isect_offsets_full"],
            int(info["width"]), int(info["height"]), int(info["tile_width"]), int(info["tile_height"]))


def composite_features(info: Dict, C_: int, N: int, table: Tensor, launch_flags: Optional[int] = None) -> Tensor:
    """[C,H,W,K] float32 = sum_i w_i table[n_i] over the lists of the colour pass that returned ``info`` (qed_features_fwd)."""
    splats, ids, offsets, w, h, tw, th = _lists(info, "composite_features")
    if not (table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2
            and table.shape[0] == N):
        raise ValueError(f"composite_features: a contiguous float32 [{N}, K] table on the GPU")
    K = int(table.shape[1])
    out = torch.empty(C_, h, w, K, dtype=torch.float32, device=table.device)
    flags = L.composite_launch_flags() if launch_flags is None else int(launch_flags)
    L.check(L.load().qed_features_fwd(C_, N, K, L.ptr(splats), L.ptr(ids), L.ptr(offsets), w, h, tw, th, L.ptr(table),
                                      L.ptr(out), flags, _stream()), "qed_features_fwd")
    return out


def composite_features_bwd(info: Dict, C_: int, N: int, v_out: Tensor, v_table: Tensor,
                           launch_flags: Optional[int] = None) -> None:
    """``v_table`` [N,K] += the gradient of ``composite_features`` for the upstream ``v_out`` [C,H,W,K] (qed_features_bwd)."""
    splats, ids, offsets, w, h, tw, th = _lists(info, "composite_features_bwd")
    K = int(v_table.shape[1])
    if not (v_out.is_contiguous() and v_out.dtype == torch.float32 and v_out.numel() == C_ * h * w * K
            and v_table.is_contiguous() and v_table.dtype == torch.float32 and v_table.shape[0] == N):
        raise ValueError("composite_features_bwd: contiguous float32 v_out [C,H,W,K] and v_table [N,K]")
    flags = L.composite_launch_flags() if launch_flags is None else int(launch_flags)
    L.check(L.load().qed_features_bwd(C_, N, K, L.ptr(splats), L.ptr(ids), L.ptr(offsets), w, h, tw, th, L.ptr(v_out),
                                      L.ptr(v_table), flags, _stream()), "qed_features_bwd")


def label_loss(logits: Tensor, labels: Tensor, ignore_label: int = 255, class_weight: Optional[Tensor] = None,
               want_grad: bool = True, workspace: Optional[Tensor] = None, loss_out: Optional[Tensor] = None):
    """``(loss [1], v_logits | None)``: ``torch.nn.functional.cross_entropy(logits, labels, weight=class_weight,
    ignore_index=ignore_label)`` of ``logits`` [..., K] float32 against ``labels`` [...] uint8, and its gradient
    (qed_label_loss).  A label >= K counts as ignored; with no labelled pixel both are 0."""
    K = int(logits.shape[-1])
    n_pix = logits.numel() // K
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous()):
        raise ValueError("label_loss: contiguous float32 logits on the GPU")
    if not (labels.dtype == torch.uint8 and labels.is_contiguous() and labels.numel() == n_pix and labels.device == logits.device):
        raise ValueError(f"label_loss: {n_pix} contiguous uint8 labels on {logits.device}")
    if class_weight is not None:
        class_weight = class_weight.to(logits.device, torch.float32).contiguous()
        if class_weight.numel() != K:
            raise ValueError(f"label_loss: {class_weight.numel()} class weights for {K} classes")
    if workspace is None:
        workspace = torch.empty(L.LABEL_LOSS_WS_DOUBLES, dtype=torch.float64, device=logits.device)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device) if loss_out is None else loss_out
    grad = torch.empty_like(logits) if want_grad else None
    L.check(L.load().qed_label_loss(n_pix, K, L.ptr(logits), L.ptr(labels), int(ignore_label), L.ptr(class_weight),
                                    L.ptr(workspace), L.ptr(grad), L.ptr(loss), _stream()), "qed_label_loss")
    return loss, grad


def label_confusion(logits: Tensor, labels: Tensor, confusion: Tensor, ignore_label: int = 255, acc: Optional[Tensor] = None,
                    min_alpha: float = 0.5) -> Tensor:
    """``confusion`` [K, K + 1] int64 (row = label, column = prediction, the last column = accumulation below ``min_alpha``)
    += the counts of one image (qed_label_confusion)."""
    K = int(logits.shape[-1])
    n_pix = logits.numel() // K
    if tuple(confusion.shape) != (K, K + 1) or confusion.dtype != torch.int64 or not confusion.is_contiguous():
        raise ValueError(f"label_confusion: a contiguous int64 [{K}, {K + 1}] table")
    if not (logits.dtype == torch.float32 and logits.is_contiguous() and labels.dtype == torch.uint8
            and labels.is_contiguous() and labels.numel() == n_pix):
        raise ValueError("label_confusion: contiguous float32 logits [..., K] and uint8 labels [...]")
    if acc is not None:
        acc = acc.reshape(-1)
        if not (acc.dtype == torch.float32 and acc.is_contiguous() and acc.numel() == n_pix):
            raise ValueError("label_confusion: acc is a contiguous float32 plane of the image's size")
    L.check(L.load().qed_label_confusion(n_pix, K, L.ptr(logits), L.ptr(labels), int(ignore_label), L.ptr(acc),
                                         float(min_alpha), L.ptr(confusion), _stream()), "qed_label_confusion")
    return confusion


def present_labels(logits: Tensor, acc: Optional[Tensor], palette: Tensor, min_alpha: float = 0.5) -> Tuple[Tensor, Tensor]:
    """``(label [H,W] uint8, rgb [H,W,3] uint8)`` of ``logits`` [H,W,K]: the argmax and its palette colour; a pixel whose
    accumulation is below ``min_alpha`` gets 255 and the palette's last row (qed_label_present)."""
    h, w, K = (int(s) for s in logits.shape)
    if tuple(palette.shape) != (K + 1, 3) or palette.dtype != torch.uint8:
        raise ValueError(f"present_labels: a [{K + 1}, 3] uint8 palette")
    palette = palette.to(logits.device).contiguous()
    if acc is not None:
        acc = acc.reshape(-1).contiguous()
    label = torch.empty(h, w, dtype=torch.uint8, device=logits.device)
    rgb = torch.empty(h, w, 3, dtype=torch.uint8, device=logits.device)
    L.check(L.load().qed_label_present(h * w, K, L.ptr(logits.contiguous()), L.ptr(acc), float(min_alpha), L.ptr(palette),
                                       L.ptr(label), L.ptr(rgb), _stream()), "qed_label_present")
    return label, rgb


# ---- on a model ------------------------------------------------------------------------------------------------------------
class _Frozen:
    """The model in evaluation mode with the records kept, the crop box off and no extra passes, as prune.score_views
    renders; everything is put back on exit."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        m = self.model
        self.saved = (m.training, m.crop_box, getattr(m.config, "output_normals", False),
                      getattr(m.config, "output_depth_spread", False))
        m.eval()
        m.crop_box = None
        m.config.output_normals = False
        m.config.output_depth_spread = False
        m.__dict__["_score_records"] = True
        return self

    def __exit__(self, *exc):
        m = self.model
        m.__dict__.pop("_score_records", None)
        training, m.crop_box, m.config.output_normals, m.config.output_depth_spread = self.saved
        m.train(training)
        return False

    def render(self, camera):
        """(info with the records, accumulation [H,W], H, W) of one view."""
        out = self.model.get_outputs(camera)
        h, w = int(out["rgb"].shape[-3]), int(out["rgb"].shape[-2])
        info = self.model.info
        if int(info["n_cameras"]) != 1:
            raise NotImplementedError("semantic: one camera per render")
        return info, out["accumulation"].reshape(h, w), h, w

    @staticmethod
    def release(info: Dict) -> None:
        info.pop("_splats", None)
        info.pop("_isect_offsets_full", None)


def _refuse(model, field: SemanticField, captured_step=None) -> None:
    field.check_model(model)
    if field.n_classes > MAX_CLASSES:
        raise ValueError(f"semantic: {field.n_classes} classes; at most {MAX_CLASSES} are offered")
    if model.device.type != "cuda" or field.device != model.device:
        raise L.QedSplatError("semantic: the model and the field live on one GPU (there is no CPU path)")
    if captured_step is not None and model.training:
        raise NotImplementedError("semantic: a model in training mode with a captured step replays launches of its own "
                                  "buffers; finish training (model.eval()) or drop the captured step first")


def _check_label(label: Tensor, h: int, w: int, k: int) -> Tensor:
    if label.numel() != h * w or label.dtype != torch.uint8:
        shape = tuple(label.shape)
        raise ValueError(f"view {k}: the label image is {shape} {label.dtype}, its frame renders {h}x{w} uint8 "
                         "(resizing is not offered)")
    return label.reshape(h, w).contiguous()


@torch.no_grad()
def render_logits(model, camera, field: SemanticField, captured_step=None) -> Tuple[Tensor, Tensor]:
    """``(logits [H,W,K], acc [H,W])`` of one view: one evaluation render with the records kept, then one
    qed_features_fwd."""
    _refuse(model, field, captured_step)
    with _Frozen(model) as fr:
        info, acc, h, w = fr.render(camera)
        logits = composite_features(info, 1, model.num_points, field.logits)[0]
        fr.release(info)
    return logits, acc


@dataclass
class FitConfig:
    """``steps`` Adam steps at ``lr``; a step averages the loss of ``views_per_step`` views drawn (with ``seed``) without
    replacement per epoch; ``class_weight`` [K] as torch's ``cross_entropy(weight=)``; ``log_every`` > 0 prints (and reads
    back) the loss every so many steps."""
    steps: int = 500
    lr: float = 0.05
    ignore_label: int = 255
    class_weight: Optional[Sequence[float]] = None
    views_per_step: int = 1
    seed: int = 0
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    log_every: int = 0


@torch.no_grad()
def fit(model, cameras: Sequence, labels: Sequence[Tensor], field: SemanticField, config: Optional[FitConfig] = None,
        captured_step=None) -> List[float]:
    """Fit the field's table so that the composited logits reproduce ``labels`` (per camera a uint8 [H,W] class map, 255 =
    unlabelled).  Per step and view: an evaluation render, qed_features_fwd, qed_label_loss, qed_features_bwd; then one
    qed_adam_step on the table.  Nothing is read back inside the loop but the optional print; the per-step losses are kept
    on the device and returned as a list after the last step."""
    cfg = config or FitConfig()
    _refuse(model, field, captured_step)
    if len(cameras) != len(labels) or not len(cameras):
        raise ValueError(f"fit: {len(cameras)} cameras and {len(labels)} label images")
    if cfg.steps < 0 or cfg.views_per_step < 1:
        raise ValueError("fit: steps >= 0 and views_per_step >= 1")
    dev, N, K = model.device, model.num_points, field.n_classes
    for k, (cam, lab) in enumerate(zip(cameras, labels)):          # before any launch
        _check_label(lab, int(cam.height.reshape(-1)[0]), int(cam.width.reshape(-1)[0]), k)
    cw = None
    if cfg.class_weight is not None:
        cw = torch.as_tensor(cfg.class_weight, dtype=torch.float32).reshape(-1).to(dev)
        if cw.numel() != K:
            raise ValueError(f"fit: {cw.numel()} class weights for {K} classes")
    lib = L.load()
    V = int(cfg.views_per_step)
    losses = torch.zeros(max(cfg.steps, 1), V, dtype=torch.float32, device=dev)
    grad = torch.zeros(N, K, dtype=torch.float32, device=dev)
    ws = torch.empty(L.LABEL_LOSS_WS_DOUBLES, dtype=torch.float64, device=dev)
    h_begin = (C.c_int64 * 2)(0, N * K)
    h_lr = (C.c_float * 1)(float(cfg.lr))
    gen = torch.Generator().manual_seed(int(cfg.seed))
    unseen: List[int] = []
    with _Frozen(model) as fr:
        for step in range(cfg.steps):
            grad.zero_()
            for v in range(V):
                if not unseen:
                    unseen = torch.randperm(len(cameras), generator=gen).tolist()
                j = unseen.pop()
                info, _, h, w = fr.render(cameras[j])
                lab = _check_label(labels[j], h, w, j).to(dev, non_blocking=True)
                logits = composite_features(info, 1, N, field.logits)
                _, v_logits = label_loss(logits, lab, cfg.ignore_label, cw, True, ws, losses[step, v:v + 1])
                composite_features_bwd(info, 1, N, v_logits, grad)
                fr.release(info)
            if V > 1:
                grad.mul_(1.0 / V)
            if N:
                field.step += 1
                L.check(lib.qed_adam_step(L.ptr(field.logits), L.ptr(grad), L.ptr(field.exp_avg), L.ptr(field.exp_avg_sq), 1,
                                          C.cast(h_begin, C.c_void_p), C.cast(h_lr, C.c_void_p), float(cfg.betas[0]),
                                          float(cfg.betas[1]), float(cfg.eps), int(field.step), None, _stream()),
                        "qed_adam_step")
            if cfg.log_every > 0 and (step + 1) % cfg.log_every == 0:
                print(f"semantic fit: step {step + 1} / {cfg.steps}  loss {float(losses[step].mean()):.6f}", flush=True)
    return losses[:cfg.steps].mean(dim=1).tolist()


def iou_from_confusion(confusion: Tensor) -> Dict:
    """``{"miou", "pixel_accuracy", "per_class_iou", "confusion"}`` of a [K, K + 1] (or [K, K]) table of counts, row =
    label, column = prediction (a last column K: no prediction).  IoU of class k = tp / (tp + fp + fn); a pixel without a
    prediction is a false negative of its label's class.  Classes absent from both the labels and the predictions are left
    out of the mean (None in ``per_class_iou``); no labelled pixel at all: miou and pixel_accuracy are 0."""
    c = confusion.detach().cpu().to(torch.int64)
    K = int(c.shape[0])
    tp = c[:, :K].diagonal()
    n_label = c.sum(dim=1)                              # tp + fn
    n_pred = c[:, :K].sum(dim=0)                        # tp + fp
    union = n_label + n_pred - tp
    per_class = [float(tp[k]) / float(union[k]) if int(union[k]) > 0 else None for k in range(K)]
    present = [v for v in per_class if v is not None]
    total = int(c.sum())
    return {"miou": sum(present) / len(present) if present else 0.0,
            "pixel_accuracy": float(tp.sum()) / total if total else 0.0,
            "per_class_iou": per_class, "confusion": c.tolist()}


@torch.no_grad()
def evaluate(model, cameras: Sequence, labels: Sequence[Tensor], field: SemanticField, min_alpha: float = 0.5,
             ignore_label: int = 255, captured_step=None) -> Dict:
    """The confusion counts of every view (qed_label_confusion: integer adds, the same bits for any order of views) and
    ``iou_from_confusion`` of them.  A pixel whose accumulation is below ``min_alpha`` has no prediction."""
    _refuse(model, field, captured_step)
    if len(cameras) != len(labels):
        raise ValueError(f"evaluate: {len(cameras)} cameras and {len(labels)} label images")
    for k, (cam, lab) in enumerate(zip(cameras, labels)):
        _check_label(lab, int(cam.height.reshape(-1)[0]), int(cam.width.reshape(-1)[0]), k)
    K = field.n_classes
    confusion = torch.zeros(K, K + 1, dtype=torch.int64, device=model.device)
    with _Frozen(model) as fr:
        for k, cam in enumerate(cameras):
            info, acc, h, w = fr.render(cam)
            logits = composite_features(info, 1, model.num_points, field.logits)
            lab = _check_label(labels[k], h, w, k).to(model.device)
            label_confusion(logits, lab, confusion, ignore_label, acc.contiguous(), min_alpha)
            fr.release(info)
    return iou_from_confusion(confusion)


# ---- command line ------------------------------------------------------------------------------------------------------------
def _labelled_items(dm, split: str, stride: int):
    items = list({"train": dm.train_items, "eval": dm.eval_items, "all": dm.all_items}[split]())
    items = [(cam, b["label"]) for cam, b in items if "label" in b][::max(int(stride), 1)]
    if not items:
        raise SystemExit(f"no frame of the {split} split has a label_path")
    return [c for c, _ in items], [lab for _, lab in items]


def read_classes_file(path):
    """``(class names, palette [K + 1, 3] uint8 or None, class weights or None)`` of a ``--classes-file``: a JSON list of
    names, or ``{"classes": [...], "palette": [[r, g, b], ...], "class_weight": [...]}``."""
    with open(path) as f:
        meta = json.load(f)
    meta = {"classes": meta} if isinstance(meta, list) else meta
    if not isinstance(meta.get("classes"), list) or not meta["classes"]:
        raise ValueError(f"{path}: a list of class names, or an object with a \"classes\" list")
    palette = torch.tensor(meta["palette"], dtype=torch.uint8) if "palette" in meta else None
    return [str(n) for n in meta["classes"]], palette, meta.get("class_weight")


def infer_n_classes(labels: Sequence[Tensor], ignore_label: int = 255) -> int:
    """The largest class value of the label images that is not ``ignore_label``, plus one (1 when nothing is labelled)."""
    top = -1
    for lab in labels:
        named = lab[lab != ignore_label]
        if named.numel():
            top = max(top, int(named.max()))
    return top + 1 if top >= 0 else 1


def main(argv=None) -> Dict:
    from .render import add_dataparser_arguments, load_model
    ap = argparse.ArgumentParser(prog="python -m qed_splatter_amd.semantic", description="Fit and evaluate per-Gaussian class logits on a trained model")
    ap.add_argument("command", choices=("fit", "eval"))
    ap.add_argument("--load", required=True, metavar="CKPT", help="a checkpoint written by train.py --save")
    ap.add_argument("--data", required=True, metavar="DIR", help="the dataset of the training run, with label_path frames")
    ap.add_argument("--output", metavar="FIELD.pt", default=None, help="fit: where the field is written")
    ap.add_argument("--field", metavar="FIELD.pt", default=None, help="eval: the field; fit: a field to go on from")
    ap.add_argument("--output-path", metavar="OUT.json", default=None, help="eval: where the metrics are written")
    ap.add_argument("--split", choices=("train", "eval", "all"), default=None, help="default: train for fit, eval for eval")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--views-per-step", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log-every", type=int, default=0)
    ap.add_argument("--min-alpha", type=float, default=0.5)
    ap.add_argument("--classes-file", metavar="JSON", default=None,
                    help='a list of class names, or {"classes": [...], "palette": [[r, g, b], ...], "class_weight": [...]}')
    ap.add_argument("--stride", type=int, default=1, help="use every S-th labelled view")
    ap.add_argument("--background-color", choices=("random", "black", "white"), default="random")
    add_dataparser_arguments(ap)
    a = ap.parse_args(argv)
    if a.undistort:
        raise SystemExit("--undistort: there is no nearest-neighbour resampling of labels yet")
    if a.command == "fit" and not a.output:
        ap.error("fit needs --output")
    if a.command == "eval" and not a.field:
        ap.error("eval needs --field")
    if not torch.cuda.is_available():
        raise SystemExit("qed_splatter_amd.semantic needs a GPU")
    from .datamanager import FullImageDatamanager
    from .dataparser import DataparserConfig
    L.load()
    device = torch.device("cuda:0")
    model, _ = load_model(a.load, device, a.background_color)
    model.eval()
    dp_cfg = DataparserConfig(orientation_method=a.orientation_method, center_method=a.center_method,
                              auto_scale_poses=a.auto_scale_poses == "True", depth_unit_scale_factor=a.depth_unit_scale_factor,
                              train_split_fraction=a.train_split_fraction, scale_factor=a.scale_factor, undistort=False)
    dm = FullImageDatamanager(a.data, dp_cfg, device=a.cache_device)
    cameras, labels = _labelled_items(dm, a.split or ("train" if a.command == "fit" else "eval"), a.stride)
    result: Dict = {"command": a.command, "views": len(cameras)}
    if a.command == "eval":
        field = SemanticField.load(a.field, device)
        result.update(evaluate(model, cameras, labels, field, a.min_alpha))
        result["class_names"] = field.class_names
        if a.output_path:
            with open(a.output_path, "w") as f:
                json.dump(result, f)
        print(json.dumps(result))
        return result
    names, palette, weight = read_classes_file(a.classes_file) if a.classes_file else (None, None, None)
    if a.field:
        field = SemanticField.load(a.field, device)
    else:
        field = SemanticField(model.num_points, len(names) if names is not None else infer_n_classes(labels), device, names,
                              palette)
    history = fit(model, cameras, labels, field, FitConfig(steps=a.steps, lr=a.lr, class_weight=weight,
                                                           views_per_step=a.views_per_step, seed=a.seed, log_every=a.log_every))
    field.save(a.output)
    result.update(steps=a.steps, n_classes=field.n_classes, first_loss=history[0] if history else None,
                  last_loss=history[-1] if history else None, output=str(a.output))
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
