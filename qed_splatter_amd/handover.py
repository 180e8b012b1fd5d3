"""What a training step's loss launch does for the compositing backward, as ONE object both sides hold.

The loss launch can zero the ``[C N, 16]`` gradient accumulator the compositing backward adds into (no fill launch there),
on the fused route sort the tiles into that backward's launch order (no ordering launch), and behind a captured
``get_outputs`` segment write ``v_rgb`` / ``v_depth`` straight into the segment's static buffers (no copies).  A
``Handover`` is made once per step by ``get_outputs`` / ``fused_loss`` -- once per captured segment by
``segments.OutputsSegment``, which re-arms it every replay -- given to ``rasterization(_handover=...)`` and to the loss
node, and says what may be handed:

  * what the producer may use: ``rows`` (C N), a segment's static ``vsplat`` / ``v_rgb`` / ``v_depth`` (None on eager
    steps) and the camera's ``FrameOrder`` (or None);
  * the one-shot claims: the FIRST loss node to ask zeroes the accumulator (``claim_accumulator``) and writes the static
    gradient buffers (``claim_grad_buffers``); a second loss on the same outputs is refused and computes in full;
  * the offer: ``offer()`` by the loss launch, ``take()`` by the compositing backward -- which empties it, so that a second
    backward through a retained graph fills its own accumulator and order, and nothing keeps the accumulator alive.

``take()`` is the one place that decides whether a handed buffer is fit for the raw pointers of ``qed_composite_bwd``.
"""
from __future__ import annotations

import torch

from . import _lib as L


class FrameOrder:
    """A camera's persistent launch-order buffer ``[tiles + 1]`` int32 (model._frame_orders): written by the launch that
    orders a frame's compositing backward, read by the compositing forward of the NEXT frame of that camera.  ``valid``
    once a launch that writes it has been enqueued."""

    __slots__ = ("buffer", "valid")

    def __init__(self, buffer):
        self.buffer, self.valid = buffer, False

    def fits(self, n_tiles: int) -> bool:
        return self.buffer.numel() == n_tiles + 1


class Handover:
    """One step's (one captured segment's) hand-over from the loss launch to the compositing backward: the module docstring."""

    __slots__ = ("rows", "frame_order", "vsplat", "v_rgb", "v_depth", "offered_vsplat", "offered_order", "_zeroes", "_writes")

    def __init__(self, rows: int = 0, frame_order: FrameOrder = None, vsplat=None, v_rgb=None, v_depth=None):
        self.rows, self.frame_order = rows, frame_order
        self.vsplat, self.v_rgb, self.v_depth = vsplat, v_rgb, v_depth       # a segment's static buffers
        self.reset()

    # ---- the loss node ----
    def claim_accumulator(self) -> bool:
        """Once: the right to zero ``accumulator()`` in the loss launch and ``offer()`` it."""
        first, self._zeroes = not self._zeroes, True
        return first and self.rows > 0

    def claim_grad_buffers(self) -> bool:
        """Once, behind a captured segment: the right to write ``v_rgb`` / ``v_depth`` (None: not rendered) in place."""
        first, self._writes = not self._writes, True
        return first and self.v_rgb is not None

    def accumulator(self, device):
        """The buffer for the claimant to zero: the segment's static one, else a fresh (uninitialised) one."""
        return self.vsplat if self.vsplat is not None else \
            torch.empty(self.rows, L.VSPLAT_FLOATS, dtype=torch.float32, device=device)

    def offer(self, vsplat=None, order=None) -> None:
        """What the launch just enqueued did: zeroed ``vsplat``, wrote the launch order ``order``.  Replaces any earlier one."""
        self.offered_vsplat, self.offered_order = vsplat, order

    # ---- the compositing backward ----
    def take(self, C: int, N: int, n_tiles: int, device):
        """(zeroed accumulator | None, launch order | None): what was offered and fits this launch; the offer is emptied."""
        vsplat, order = self.offered_vsplat, self.offered_order
        self.offer()
        fit = vsplat is not None and vsplat.shape == (C * N, L.VSPLAT_FLOATS) and vsplat.device == device \
            and vsplat.dtype == torch.float32
        return vsplat if fit else None, order if (order is not None and order.numel() == n_tiles + 1) else None

    # ---- a captured segment ----
    def take_static_zeroed(self) -> bool:
        """Before a replay of the captured backward: did the loss launch zero the STATIC accumulator?  Empties the offer."""
        hit = self.offered_vsplat is not None and self.offered_vsplat is self.vsplat
        self.offer()
        return hit

    def reset(self) -> None:
        """A new replay of the segment: no offer, both claims open."""
        self.offer()
        self._zeroes = self._writes = False
