"""The compact form of the SH gradients.  The 48 coefficient gradients of a Gaussian are b_k(direction to the camera) x
colour gradient, so a backward pass may leave only the clamp-masked colour gradient of its view in ``features_dc.grad`` and
the active rows of ``features_rest.grad`` unwritten; ``qed_adam_step_sh`` evaluates the product inside the optimiser pass,
``qed_sh_grad_from_views`` writes it out.  A model says so with ONE attribute, ``compact_sh``: the ``CompactSHGrad`` of the
backward pass that wrote the fields, None exactly when they hold full gradients.  The record belongs to that backward pass
and to the fields, not to a forward call (``QEDSplatterModel._resolve_sh_grad``); a step captured into a hipGraph makes it
once, at capture, and nothing on a replay path clears it."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib as L


class SHViews(NamedTuple):
    """What both entry points build the coefficient gradients from: ``n_views`` view matrices ``vm_stride`` floats apart,
    as many colour gradients [3 N] ``grad_stride`` floats apart, and the weight of each view."""
    n_views: int
    viewmats: Tensor
    vm_stride: int
    grads: Tensor
    grad_stride: int
    scale: float

    @classmethod
    def own(cls, viewmat: Tensor, v_color: Tensor) -> "SHViews":
        """This rank's view alone: its view matrix and the colour gradient its backward pass left."""
        return cls(1, viewmat, 16, v_color, 0, 1.0)

    @classmethod
    def rows(cls, buf: Tensor, nv: int) -> "SHViews":
        """The rows of a message buffer [R, row] (parallel.py: 3 N colour gradients, then the view matrix), averaged."""
        return cls(buf.shape[0], buf[:, nv:], buf.shape[1], buf, buf.shape[1], 1.0 / buf.shape[0])

    def c_args(self) -> tuple:
        """(n_views, viewmats, viewmat_stride, v_views, view_stride, scale) as qed_adam_step_sh takes them."""
        return (self.n_views, L.ptr(self.viewmats), self.vm_stride, L.ptr(self.grads), self.grad_stride, float(self.scale))


def write_sh_grads(means: Tensor, views: SHViews, sh_degree: int, out_dc: Tensor, out_rest: Tensor) -> None:
    """``out_dc`` [N,3] receives the gradient of features_dc, ``out_rest`` [N,KR,3] the active coefficients' gradients,
    averaged over ``views`` -- in place when ``out_dc`` is the one view's colour gradient itself."""
    n = means.shape[0]
    rest_w = out_rest.numel() // max(n, 1)
    assert 3 * ((int(sh_degree) + 1) ** 2 - 1) <= rest_w
    with torch.no_grad():
        # (a single view's stride is never stepped over, but this entry point wants every stride to span a view)
        L.check(L.load().qed_sh_grad_from_views(
            n, views.n_views, L.ptr(means), L.ptr(views.viewmats), views.vm_stride, L.ptr(views.grads),
            max(views.grad_stride, 3 * n), int(sh_degree), float(views.scale), L.ptr(out_dc), 3, L.ptr(out_rest), rest_w,
            L.current_stream()), "qed_sh_grad_from_views")


class CompactSHGrad:
    """What one backward pass left in place of the full SH gradients: its view matrix and active degree, and
      * implicit (``config.lazy_sh_grad``: nobody asked, so every Python reader of ``.grad`` must still see full gradients):
        detached ALIASES ``v_color`` / ``v_rest`` of the two fields -- never the gradient tensors themselves: the engine
        adopts an incoming gradient without a copy only while nobody else holds that object -- and the means' identity;
      * explicit (``fused_loss(compact_sh_grad=True)``: the caller consumes it, reading ``.grad`` does not write out): the
        ``views`` a compact exchange gathered (parallel.py), None for this rank's view only."""

    __slots__ = ("viewmat", "deg", "implicit", "v_color", "v_rest", "n", "means_version", "means_ptr", "views")

    def __init__(self, viewmat: Optional[Tensor], deg: int, implicit: bool = False, v_color: Optional[Tensor] = None,
                 v_rest: Optional[Tensor] = None, means: Optional[Tensor] = None):
        self.viewmat, self.deg, self.implicit, self.views = viewmat, int(deg), implicit, None
        self.v_color = self.v_rest = self.n = self.means_version = self.means_ptr = None
        if v_color is not None:
            self.v_color, self.v_rest, self.n = v_color.detach(), v_rest.detach(), int(v_color.shape[0])
            self.means_version, self.means_ptr = means._version, means.data_ptr()

    def optimiser_views(self, flat_grad: Optional[Tensor] = None, group_begin=None) -> SHViews:
        """The views the optimiser pass reads: the gathered ones, else this rank's own colour gradient -- the alias an
        implicit record keeps, the features_dc range of ``flat_grad`` for an explicit one."""
        if self.views is not None:
            return self.views
        own = self.v_color if self.implicit else flat_grad[group_begin[-3]:group_begin[-2]]
        return SHViews.own(self.viewmat, own)

    def write_out(self, model, flat_grad: Optional[Tensor] = None) -> None:
        """End the record: write the coefficient gradients it stands for into the very allocation the ``.grad`` fields
        view (features_dc: b_0 x colour gradient in place of the colour gradient; features_rest: the active coefficients)."""
        model.__dict__["compact_sh"] = None
        means = model.gauss_params["means"]
        if not self.implicit:
            g = flat_grad if flat_grad is not None else model.flat_grad()
            (dc, rest), (_, end) = model.layout.span("features_dc"), model.layout.span("features_rest")
            return write_sh_grads(means, self.optimiser_views(g, model.group_begin), self.deg, g[dc:rest], g[rest:end])
        if means._version != self.means_version or means.data_ptr() != self.means_ptr or means.shape[0] != self.n:
            raise RuntimeError(
                "lazy SH gradients: the means were modified after the backward pass and before the gradients of features_dc "
                "/ features_rest were read (the SH basis is evaluated at the means of the forward pass).  Step all six groups "
                "with QedAdam, read the gradients before stepping, or set config.lazy_sh_grad = False")
        write_sh_grads(means, self.optimiser_views(), self.deg, self.v_color, self.v_rest)


def explicit_record(model) -> Optional[CompactSHGrad]:
    """The model's record if a ``fused_loss(compact_sh_grad=True)`` backward pass wrote the fields, else None."""
    rec = model.__dict__.get("compact_sh")
    return rec if rec is not None and not rec.implicit else None
