"""The reference's data manager -- ``FullImageDatamanager[DepthDataset]`` with ``cache_images_type="uint8"``
(config.py:34-38) -- over ``dataparser.parse_dataset``: every frame is loaded once and cached as the files store it
(uint8 colour, RGBA kept; 16-bit depth as uint16 with ONE scalar; bool masks; uint8 class maps under ``"label"`` [H,W] for
the frames of a dataset that has them, semantic.py), and every training step is handed a
different camera and that camera's cached frame.  The float ground truth the loss kernels read is made per step by
``QEDSplatterModel._ground_truth`` (csrc/ingest.hip, one launch): it depends on the step's downscale factor and on
the step's background colour, so it cannot be made here.

``GpuBatch`` and 16-bit depth.  The batch keeps the reference's keys (``image``, ``depth_image``, optional ``mask``,
``image_idx``) plus ``depth_scale``.  For a 16-bit depth file the cached tensor is uint16 and ``depth_scale`` =
``depth_unit_scale_factor * dataparser_scale``; the ingest kernel reads it raw (``batch.raw("depth_image")``).  Every
other reader -- ``get_metrics_dict``, ``get_loss_dict`` on a batch that does not qualify for the kernel, user code --
indexes the batch, and ``batch["depth_image"]`` (and ``.get``) hand out a float32 view in metres, made on first use
and kept for the life of the batch object (one step): ``uint16.float() * depth_scale``, which is also, bit for bit,
what the kernel computes at full resolution.  ``items()`` / ``values()`` show the stored tensors.

Distorted cameras (``DataparserConfig.undistort``).  A frame with non-zero coefficients or the fisheye model is
resampled to the dataparser's new pinhole once, by ``undistort_frame`` (csrc/undistort.hip, one launch over all of its
planes on the compute device), before it enters the cache; a ``device="cpu"`` cache gets the result copied back.  The
cached planes keep their dtypes (uint16 depth stays uint16).  Frames without distortion take the path they always
took.  There is no CPU implementation: without a GPU a distorted frame raises ``QedSplatError``.
"""
from __future__ import annotations

import copy
import ctypes
from pathlib import Path
from typing import Iterator, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .dataparser import DataparserConfig, DataparserOutputs, parse_dataset
from .init_pointcloud import load_color_u8, load_depth
from .model import PinholeCameras
from .undistort import is_distorted, model_code


class GpuBatch(dict):
    """A training batch whose tensors are the cached frame as stored (see the module docstring).  A plain ``dict`` for
    every consumer; only ``depth_image`` is special when it is stored as uint16."""

    def raw(self, key):
        """The stored tensor (uint16 for 16-bit depth), without conversion."""
        return dict.__getitem__(self, key)

    def _depth_f32(self) -> Tensor:
        d = self.__dict__.get("_f32")
        if d is None:
            d = self.__dict__["_f32"] = dict.__getitem__(self, "depth_image").float() * float(dict.get(self, "depth_scale", 1.0))
        return d

    def __getitem__(self, key):
        v = dict.__getitem__(self, key)
        if key == "depth_image" and v.dtype == torch.uint16:
            return self._depth_f32()
        return v

    def get(self, key, default=None):
        return self[key] if key in self else default

    def as_dict(self) -> dict:
        """The equivalent plain dict: float32 depth in metres, no ``depth_scale``."""
        out = {k: self[k] for k in self}
        out.pop("depth_scale", None)
        return out


def ingest_ground_truth(image: Tensor, depth: Tensor, mask: Optional[Tensor], background: Tensor, d: int,
                        depth_scale: float = 1.0):
    """(gt_rgb [Ho,Wo,3], gt_depth [Ho,Wo,1], mask [Ho,Wo,1] | None), float32, from a cached frame in one launch
    (qed_ingest_ground_truth, csrc/ingest.hip): ``d x d`` box means with Ho = H // d, Wo = W // d.  ``image`` [H,W,3|4]
    uint8 (scaled by 1/255) or float32, RGBA composited onto ``background`` [3] AFTER averaging; ``depth`` [H,W(,1)]
    uint16 (times ``depth_scale``) or float32, or None (no depth plane: gt_depth is None); ``mask`` [H,W(,1)] bool or
    None.  Contiguous tensors on one GPU, launched on the current stream of the current device."""
    dev = image.device
    if not (image.is_cuda and image.is_contiguous() and image.dim() == 3 and image.dtype in (torch.uint8, torch.float32)):
        raise ValueError("image: a contiguous uint8 or float32 [H,W,C] tensor on the GPU")
    h, w, ch = image.shape
    for name, t, dtypes in (("depth", depth, (torch.uint16, torch.float32)), ("mask", mask, (torch.bool,))):
        if t is not None and not (t.device == dev and t.is_contiguous() and t.dtype in dtypes and t.numel() == h * w):
            raise ValueError(f"{name}: a contiguous tensor of {h * w} values on {dev}, one of {dtypes}")
    bg = background
    if not (bg.dtype == torch.float32 and bg.device == dev and bg.is_contiguous()):
        bg = bg.to(dev, torch.float32).contiguous()
    if bg.numel() != 3:
        raise ValueError("background: 3 values")
    d = int(d)
    ho, wo = (h // d, w // d) if d > 0 else (0, 0)
    gt_rgb = torch.empty(ho, wo, 3, dtype=torch.float32, device=dev)
    gt_depth = torch.empty(ho, wo, 1, dtype=torch.float32, device=dev) if depth is not None else None
    gt_mask = torch.empty(ho, wo, 1, dtype=torch.float32, device=dev) if mask is not None else None
    L.check(L.load().qed_ingest_ground_truth(
        h, w, d, L.ptr(image), ch, int(image.dtype == torch.float32), L.ptr(depth),
        int(depth is not None and depth.dtype == torch.float32), float(depth_scale), L.ptr(mask), L.ptr(bg), L.ptr(gt_rgb),
        L.ptr(gt_depth), L.ptr(gt_mask), L.current_stream()), "qed_ingest_ground_truth")
    return gt_rgb, gt_depth, gt_mask


def undistort_frame(image: Tensor, depth: Optional[Tensor], mask: Optional[Tensor], src_K, new_K, dist, model,
                    return_coords: bool = False):
    """(image, depth, mask) of a distorted frame resampled to the pinhole ``new_K``, in one launch (qed_undistort_frame,
    csrc/undistort.hip; the map is defined in undistort.py).  ``image`` [H,W,3|4] uint8: bilinear with zeros outside the
    source, rounded half up; ``depth`` [H,W(,1)] uint16 or float32 and ``mask`` [H,W(,1)] bool, or None: the nearest tap,
    0 / False outside.  ``src_K`` / ``new_K`` = (fx, fy, cx, cy) and ``dist`` = (k1, k2, k3, k4, p1, p2) are host values,
    rounded to float32; ``model`` is the camera_model string.  Contiguous tensors on one GPU, launched on the current
    stream of the current device; shapes and dtypes are kept.  ``return_coords``: a fourth result, the source position
    (u, v) of every output pixel [H,W,2] float32."""
    dev = image.device
    if not (image.is_cuda and image.is_contiguous() and image.dim() == 3 and image.dtype == torch.uint8):
        raise ValueError("image: a contiguous uint8 [H,W,C] tensor on the GPU")
    h, w, ch = image.shape
    for name, t, dtypes in (("depth", depth, (torch.uint16, torch.float32)), ("mask", mask, (torch.bool,))):
        if t is not None and not (t.device == dev and t.is_contiguous() and t.dtype in dtypes and t.numel() == h * w):
            raise ValueError(f"{name}: a contiguous tensor of {h * w} values on {dev}, one of {dtypes}")
    arrays = [(ctypes.c_float * n)(*(float(v) for v in vals)) for n, vals in ((4, src_K), (4, new_K), (6, dist))]
    out_image = torch.empty_like(image)
    out_depth = torch.empty_like(depth) if depth is not None else None
    out_mask = torch.empty_like(mask) if mask is not None else None
    coords = torch.empty(h, w, 2, dtype=torch.float32, device=dev) if return_coords else None
    L.check(L.load().qed_undistort_frame(
        h, w, L.ptr(image), ch, L.ptr(depth), int(depth is not None and depth.dtype == torch.float32), L.ptr(mask),
        *arrays, model_code(model), L.ptr(out_image), L.ptr(out_depth), L.ptr(out_mask), L.ptr(coords),
        L.current_stream()), "qed_undistort_frame")
    return (out_image, out_depth, out_mask, coords) if return_coords else (out_image, out_depth, out_mask)


def _load_image(path: Path) -> np.ndarray:
    """uint8 [H,W,3], or [H,W,4] when the file has an alpha channel."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in ("RGBA", "LA", "PA") or (im.mode == "P" and "transparency" in im.info):
            return np.array(im.convert("RGBA"), dtype=np.uint8)
    rgb = load_color_u8(path)
    if rgb is None:
        raise FileNotFoundError(path)
    return rgb


def _load_depth(path: Path, unit_scale: float):
    """(array [H,W], depth_scale): a 16-bit integer image stays uint16 with ``depth_scale = unit_scale``; anything else
    (``.npy`` / ``.npz``, float images) is float32 already multiplied by it, with ``depth_scale`` 1."""
    path = Path(path)
    if path.suffix.lower() not in {".npy", ".npz"}:
        from PIL import Image
        with Image.open(path) as im:
            if im.mode in ("I;16", "I;16L", "I;16B", "I;16N"):
                return np.array(im).astype(np.uint16), float(unit_scale)
            if im.mode == "I":
                a = np.array(im)
                if a.min() >= 0 and a.max() <= 65535:
                    return a.astype(np.uint16), float(unit_scale)
    return (load_depth(path) * np.float32(unit_scale)).astype(np.float32), 1.0


def _load_mask(path: Path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("L")) != 0


def _load_label(path: Path) -> np.ndarray:
    """uint8 [H,W]: the class of every pixel as the file stores it (255 = unlabelled).  Only 8-bit greyscale images (PIL mode
    "L"): a palette image's indices name colours, not classes, and are refused like a colour image."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode != "L":
            raise ValueError(f"{path}: a label image is an 8-bit single-channel greyscale PNG (value = class), not mode "
                             f"{im.mode!r}")
        return np.array(im, dtype=np.uint8)


class FullImageDatamanager:
    """``next_train(step) -> (camera, batch)`` over the training split, ``next_eval`` / ``eval_items()`` over the
    evaluation split.

    ``device``: where the cache lives -- the GPU by default; ``"cpu"`` keeps it in (pinned, when a GPU is present) host
    memory and copies one frame per step without blocking.  ``compute_device``: where cameras and batches are handed out
    (default: the GPU when there is one, else the CPU).

    The cameras are built once and never handed out themselves: every call returns a copy, as Nerfstudio's datamanager
    does.  ``_camera_inputs`` rescales the camera it is given by 1 / d and back by d around a training step, in place and
    with integer truncation (a width of 1297 comes back as 1296 at d = 4); on a shared object that drift would stay."""

    def __init__(self, data, config: Optional[DataparserConfig] = None, device=None, compute_device=None, seed: int = 0,
                 verbose: bool = True):
        self.outputs: DataparserOutputs = data if isinstance(data, DataparserOutputs) else parse_dataset(data, config, verbose)
        have_gpu = torch.cuda.is_available()
        self.compute_device = torch.device(compute_device if compute_device is not None else ("cuda:0" if have_gpu else "cpu"))
        self.device = torch.device(device) if device is not None else self.compute_device
        self.seed = int(seed)
        self._gen = torch.Generator().manual_seed(self.seed)
        self._unseen: List[int] = []
        self._eval_next = 0
        out = self.outputs
        self.i_train = [int(i) for i in out.i_train]
        self.i_eval = [int(i) for i in out.i_eval]
        pin = self.device.type == "cpu" and self.compute_device.type == "cuda"
        unit = out.depth_unit_scale_factor * out.dataparser_scale
        self.frames: List[dict] = []
        n_bytes = 0
        labels = out.label_filenames
        if labels is not None and out.config.undistort:
            raise NotImplementedError("label images on a dataset parsed with undistort=True: there is no nearest-neighbour "
                                      "resampling of labels yet")
        for k in range(len(out)):
            img = _load_image(out.image_filenames[k])
            depth, depth_scale = _load_depth(out.depth_filenames[k], unit)
            if depth.shape[:2] != img.shape[:2]:
                raise ValueError(f"{out.depth_filenames[k]}: depth is {depth.shape[1]}x{depth.shape[0]}, its image "
                                 f"{out.image_filenames[k]} is {img.shape[1]}x{img.shape[0]} (resizing is not offered)")
            frame = {"image": torch.from_numpy(np.ascontiguousarray(img)),
                     "depth_image": torch.from_numpy(np.ascontiguousarray(depth))[..., None],
                     "depth_scale": depth_scale}
            if out.mask_filenames[k] is not None:
                mask = _load_mask(out.mask_filenames[k])
                if mask.shape[:2] != img.shape[:2]:
                    raise ValueError(f"{out.mask_filenames[k]}: mask is {mask.shape[1]}x{mask.shape[0]}, its image is "
                                     f"{img.shape[1]}x{img.shape[0]} (resizing is not offered)")
                frame["mask"] = torch.from_numpy(np.ascontiguousarray(mask))[..., None]
            if labels is not None and labels[k] is not None:
                label = _load_label(labels[k])
                if label.shape[:2] != img.shape[:2]:
                    raise ValueError(f"{labels[k]}: label image is {label.shape[1]}x{label.shape[0]}, its image is "
                                     f"{img.shape[1]}x{img.shape[0]} (resizing is not offered)")
                frame["label"] = torch.from_numpy(np.ascontiguousarray(label))
            if out.distortion_params is not None and is_distorted(out.distortion_params[k], out.camera_models[k]):
                self._undistort(frame, k)
            for key in ("image", "depth_image", "mask", "label"):
                if key in frame:
                    t = frame[key].to(self.device)
                    frame[key] = t.pin_memory() if pin else t
                    n_bytes += t.numel() * t.element_size()
            self.frames.append(frame)
        self.cache_bytes = n_bytes
        if verbose:
            print(f"datamanager: cached {len(self.frames)} frames ({len(self.i_train)} train, {len(self.i_eval)} eval), "
                  f"{n_bytes} bytes on {self.device}")
        c2w = out.camera_to_worlds.to(self.compute_device)
        self._train_cameras = [self._camera(c2w, k, j) for j, k in enumerate(self.i_train)]
        self._eval_cameras = [self._camera(c2w, k, j) for j, k in enumerate(self.i_eval)]

    def _undistort(self, frame: dict, k: int) -> None:
        """The planes of frame ``k``, as loaded, replaced by their resampling to the dataparser's new pinhole."""
        o = self.outputs
        if self.compute_device.type != "cuda":
            raise L.QedSplatError(f"{o.image_filenames[k]}: a distorted frame is undistorted on the GPU and there is none "
                                  "(there is no CPU path)")
        planes = [frame[key].to(self.compute_device) if key in frame else None for key in ("image", "depth_image", "mask")]
        with torch.cuda.device(self.compute_device):
            planes = undistort_frame(*planes, o.src_intrinsics[k], (o.fx[k], o.fy[k], o.cx[k], o.cy[k]),
                                     o.distortion_params[k], o.camera_models[k])
        for key, t in zip(("image", "depth_image", "mask"), planes):
            if t is not None:
                frame[key] = t

    def _camera(self, c2w: Tensor, k: int, idx: int) -> PinholeCameras:
        o = self.outputs
        cam = PinholeCameras(c2w[k:k + 1].contiguous(), float(o.fx[k]), float(o.fy[k]), float(o.cx[k]), float(o.cy[k]),
                             int(o.widths[k]), int(o.heights[k]), metadata={"cam_idx": idx})
        cam.intrinsics_fxfycxcy()              # (made once here: the copies of a full-resolution step share it)
        return cam

    @staticmethod
    def _hand_out(cam: PinholeCameras) -> PinholeCameras:
        """A copy of a cached camera.  Shallow is enough: rescale_output_resolution REBINDS the attributes of the object
        it is called on (``self.fx = self.fx * s``), it never writes into the tensors, so the cached camera keeps its own."""
        out = copy.copy(cam)
        out.metadata = dict(cam.metadata)
        return out

    @property
    def num_train(self) -> int:
        return len(self.i_train)

    @property
    def num_eval(self) -> int:
        return len(self.i_eval)

    def _batch(self, k: int, idx: int) -> GpuBatch:
        frame = self.frames[k]
        batch = GpuBatch()
        for key in ("image", "depth_image", "mask", "label"):
            if key in frame:
                batch[key] = frame[key].to(self.compute_device, non_blocking=True)
        batch["image_idx"] = idx
        batch["depth_scale"] = frame["depth_scale"]
        return batch

    def next_train(self, step: int = 0) -> Tuple[PinholeCameras, GpuBatch]:
        """The next training camera and its frame: every camera once per epoch, each epoch in a fresh random order
        drawn from this manager's own seeded generator (the reference pops a random index without replacement)."""
        if not self._unseen:
            self._unseen = torch.randperm(len(self.i_train), generator=self._gen).tolist()
        j = self._unseen.pop()
        return self._hand_out(self._train_cameras[j]), self._batch(self.i_train[j], j)

    def next_eval(self, step: int = 0) -> Tuple[PinholeCameras, GpuBatch]:
        """The evaluation frames in order, round and round."""
        if not self.i_eval:
            raise IndexError("the evaluation split is empty")
        j = self._eval_next
        self._eval_next = (j + 1) % len(self.i_eval)
        return self._hand_out(self._eval_cameras[j]), self._batch(self.i_eval[j], j)

    def eval_items(self) -> Iterator[Tuple[PinholeCameras, GpuBatch]]:
        for j, k in enumerate(self.i_eval):
            yield self._hand_out(self._eval_cameras[j]), self._batch(k, j)

    def train_items(self) -> Iterator[Tuple[PinholeCameras, GpuBatch]]:
        """The training frames in the split's order (``next_train`` shuffles them; this does not touch its state)."""
        for j, k in enumerate(self.i_train):
            yield self._hand_out(self._train_cameras[j]), self._batch(k, j)

    def all_items(self) -> Iterator[Tuple[PinholeCameras, GpuBatch]]:
        """Both splits in the dataset's frame order; ``image_idx`` stays the frame's index within its own split."""
        rows = [(k, self._train_cameras[j], j) for j, k in enumerate(self.i_train)]
        rows += [(k, self._eval_cameras[j], j) for j, k in enumerate(self.i_eval)]
        for k, cam, j in sorted(rows, key=lambda row: row[0]):
            yield self._hand_out(cam), self._batch(k, j)
