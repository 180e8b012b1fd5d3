"""The flat parameter layout: all six Gaussian parameter groups live back to back, in ``GROUP_ORDER``, in ONE contiguous
float32 buffer; the gradient of the projection backward and both Adam moments follow the same layout.  ``FlatLayout`` is
that contract for N Gaussians -- the model, the optimisers, densification, MCMC, the seeder and the PLY importer read
offsets, shapes, views and the kernels' ``const int64_t* begin`` argument from it instead of deriving them again."""
from __future__ import annotations

import ctypes as C

import torch

GROUP_ORDER = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
_GEOMETRY_WIDTHS = (3, 3, 4, 1)               # floats per Gaussian of means, scales, quats, opacities


def group_widths(sh_degree: int):
    """Floats per Gaussian of the six groups at ``sh_degree``."""
    return _GEOMETRY_WIDTHS + (3, 3 * ((int(sh_degree) + 1) ** 2 - 1))


class FlatLayout:
    """``n`` Gaussians with ``widths`` floats each per group: ``begin`` (the 7 offsets, the end included), ``total``,
    ``shapes`` (``(n, w)``; features_rest ``(n, w / 3, 3)``) and the begins as the ctypes array the kernels take
    (``c_begin``; ``c_begin_ptr``: cast to ``c_void_p``).  Immutable, equal by ``(n, widths)``."""

    __slots__ = ("n", "widths", "begin", "total", "shapes", "c_begin", "c_begin_ptr", "_strided")
    _CACHE: dict = {}

    def __init__(self, n: int, widths):
        self.n, self.widths = int(n), tuple(int(w) for w in widths)
        assert len(self.widths) == len(GROUP_ORDER) and self.n >= 0 and self.widths[5] % 3 == 0
        self.begin = [0]
        for w in self.widths:
            self.begin.append(self.begin[-1] + self.n * w)
        self.total = self.begin[-1]
        self.shapes = tuple((self.n, w) for w in self.widths[:5]) + ((self.n, self.widths[5] // 3, 3),)
        self.c_begin = (C.c_int64 * len(self.begin))(*self.begin)
        self.c_begin_ptr = C.cast(self.c_begin, C.c_void_p)
        # views(): (name, shape, stride, offset) of each group -- one as_strided per group, not a slice plus a view
        self._strided = tuple((name, s, (max(w, 1), 1) if len(s) == 2 else (max(w, 3), 3, 1), b)
                              for name, s, w, b in zip(GROUP_ORDER, self.shapes, self.widths, self.begin))

    @classmethod
    def with_sh_widths(cls, n: int, w_sh0: int, w_shN: int) -> "FlatLayout":
        """The four geometry groups ahead of ``w_sh0`` and ``w_shN`` colour floats, from a small cache (the projection
        backward asks every step)."""
        key = (n, w_sh0, w_shN)
        if key not in cls._CACHE:
            if len(cls._CACHE) >= 16:
                cls._CACHE.clear()
            cls._CACHE[key] = cls(n, _GEOMETRY_WIDTHS + key[1:])
        return cls._CACHE[key]

    @classmethod
    def for_sh_degree(cls, n: int, sh_degree: int) -> "FlatLayout":
        return cls(n, group_widths(sh_degree))

    @classmethod
    def of(cls, tensors) -> "FlatLayout":
        """The layout of six tensors by name.  The widths come from the shapes, so N = 0 is no special case."""
        return cls(tensors["means"].shape[0], [tensors[name].shape[1:].numel() for name in GROUP_ORDER])

    def resized(self, n: int) -> "FlatLayout":
        return FlatLayout(n, self.widths)

    def __eq__(self, other):
        return isinstance(other, FlatLayout) and (self.n, self.widths) == (other.n, other.widths)

    def __hash__(self):
        return hash((self.n, self.widths))

    def __reduce__(self):                     # (copies of a model: rebuilt, a ctypes pointer cannot be copied)
        return FlatLayout, (self.n, self.widths)

    def span(self, name: str):
        """``(lo, hi)`` of group ``name`` in the flat buffer."""
        i = GROUP_ORDER.index(name)
        return self.begin[i], self.begin[i + 1]

    def views(self, flat: torch.Tensor) -> dict:
        """name -> the group's shaped view of ``flat`` (1-D, contiguous, ``total`` elements)."""
        base = flat.storage_offset()
        return {name: flat.as_strided(shape, stride, base + b) for name, shape, stride, b in self._strided}

    def empty(self, device) -> torch.Tensor:
        return torch.empty(self.total, dtype=torch.float32, device=device)

    def empty_like_state(self, device):
        """Fresh ``(params, exp_avg, exp_avg_sq)`` buffers: what a change of N allocates."""
        return self.empty(device), self.empty(device), self.empty(device)

    def aliases(self, flat, tensors) -> bool:
        """Are the six ``tensors`` (in GROUP_ORDER) contiguous float32 views, in order, of ``flat`` -- a 1-D tensor of
        ``total`` floats, or the address of its first element?  (An empty group has no address to compare: torch gives
        every empty tensor the data_ptr 0.)"""
        if isinstance(flat, torch.Tensor):
            if not (flat.dtype == torch.float32 and flat.is_contiguous() and flat.numel() == self.total):
                return False
            flat = flat.data_ptr()
        return all(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == hi - lo and t.device == tensors[0].device
                   and (hi == lo or t.data_ptr() == flat + 4 * lo)
                   for t, lo, hi in zip(tensors, self.begin[:-1], self.begin[1:]))

    def clipped_begin(self, lo: int, hi: int):
        """The begins of the range ``[lo, hi)`` of the flat buffer, seen from ``lo``, as a ctypes array."""
        return (C.c_int64 * len(self.begin))(*[min(max(b - lo, 0), hi - lo) for b in self.begin])
