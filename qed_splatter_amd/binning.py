"""The intersection buffer of a device and the host protocol around ``qed_bin_tiles``: its capacity (calibrated per shape),
how a frame's ``{M, overflow, watchdog}`` reaches the host (at once, or one call late through pinned memory) and what follows
an overflow.  The operator (rasterization.py), its captured forms (segments.py, graph.py), the optimisers and the data-parallel
exchange (the overflow word as ``skip_flag``: optim.py, parallel.py) and model.py all go through their device's ``_Workspace``.
"""
from __future__ import annotations

import time
import warnings
import weakref
from typing import Dict

import torch

from . import _lib as L


def pinned_slot():
    """A pinned 4-word buffer that qed_bin_tiles' last list kernel stores {M, overflow, watchdog, 0} into (``host_words``), as
    (numpy view, device address, the tensor that keeps the memory alive).  The address is the one the KERNEL stores to: the
    runtime's device-side alias of the pinned block (the same number under unified addressing, but not for registered memory)."""
    import ctypes
    host = torch.zeros(4, dtype=torch.int32).pin_memory()
    dptr = ctypes.c_void_p()
    L.check(L.load().qed_host_device_pointer(host.data_ptr(), ctypes.addressof(dptr)), "qed_host_device_pointer")
    return host.numpy(), dptr.value, host


class _Workspace:
    """Per-device state that persists across calls: the status words and the intersection capacity.

    Key/value buffers are taken from PyTorch's caching allocator per call (sized by a capacity that only grows) and stay
    alive until that call's backward has run.  The kernels read the actual count M from device memory, so launches never
    need M on the host.

    The capacity is calibrated per SHAPE ``(width, height, N, C)``: the first call of a shape reads M back (one host
    read) whatever the caller asked for -- the reference's resolution schedule quadruples the pixel count at steps 3000
    and 6000 (model.py:244-250) and every densification changes N (config.py:40-41), and either can multiply M.  Calls
    of a calibrated shape may run without the read-back (``_sync=False``); their M still comes back, one call late
    (``poll_pending``), and keeps the capacity at ``HEADROOM`` x the longest list seen.  Should a frame overflow all
    the same, it renders empty, the status word makes the optimiser launches enqueued behind it no-ops
    (``qed_adam_step*``'s ``skip_flag``), and the next call regrows the buffer, warns and reads M back again: no
    exception a step late, no update from an empty frame.
    """

    HEADROOM = 2.0          # capacity / longest list seen: grids are sized by it but only M entries are ever touched
    POLL_TIMEOUT_S = 20.0   # how long poll_pending waits for a frame's count before it asks the device what happened

    def __init__(self, device):
        self.device = device
        self.capacity = 0
        # [M of the last binning call | status words]: adjacent, so that one copy reads them back (read_words)
        self.words = torch.zeros(1 + L.STATUS_WORDS, dtype=torch.int32, device=device)
        self.n_isect = self.words[:1]
        self.status = self.words[1:]
        self.overflow_word = self.words[1:2]  # int32[1] view of status[0] (non-zero: the frame just rendered overflowed and is empty)
        self._ring, self._ring_at = [], 0     # pinned read-back buffers of the asynchronous calls, reused
        self.pending = None          # (pinned host words [M, overflow, watchdog, 0], shape key, frame) of an async call
        self.frame = 0               # counts the asynchronous frames armed on this device (arm_pending)
        self.last_overflow = False   # an asynchronous frame overflowed and nobody has been told yet (take_overflow_flag)
        self.m_seen: Dict[tuple, int] = {}   # shape key -> longest list read back for that shape
        self.force_sync = False      # the next call reads M back (an asynchronous frame overflowed)
        self.overflows = 0           # asynchronous frames that rendered empty (diagnostics / tests)
        # optimisers that keep a HOST step counter and take this workspace's overflow word as skip_flag: told when a step
        # was skipped on the device, so that their bias corrections stay in step with their moments
        self.steppers: "weakref.WeakSet" = weakref.WeakSet()
        self.waited_s = 0.0          # host time spent in poll_pending waiting for the device to reach the previous frame's binning
        self.host_words_ok = True    # False once a count failed to arrive through pinned memory: read-backs by copy from then on

    def host_slot(self):
        """A pinned_slot() for one asynchronous read-back, as (numpy view, address): ``poll_pending`` watches word 0 turn
        from -1 into M.  Neither a copy nor an event enters the stream: the 12-byte device-to-host copy and the event that
        used to sit behind the binning cost ~10 us between it and the compositing pass (a blit kernel and two barrier
        packets).  At most one read-back is pending at a time (the next call polls it before it arms its own), so two
        slots used in turn are never overwritten in flight."""
        if not self._ring:
            self._ring = [pinned_slot(), pinned_slot()]
        self._ring_at ^= 1
        words, ptr, _keep = self._ring[self._ring_at]
        words[0] = -1
        return words, ptr

    def reset(self) -> None:
        """Forget every calibration (the next call of any shape reads M back and sizes the buffer afresh)."""
        self.poll_pending()
        self.capacity, self.m_seen, self.force_sync = 0, {}, False

    def may_capture(self, key) -> bool:
        """Has a synchronous call sized the buffer for this shape?  (What a hipGraph capture asks: force_sync is not its concern.)"""
        return self.capacity > 0 and key in self.m_seen

    def may_skip_readback(self, key) -> bool:
        """May a call of this shape run without reading M back?  (Not its first call, nor the call after an overflow.)"""
        return self.capacity > 0 and key in self.m_seen and not self.force_sync and self.host_words_ok

    def saw(self, key, M: int) -> None:
        """A call of shape ``key`` (None: of a shape nobody keeps a record for) needed M entries: make room for it."""
        if key is not None:
            self.m_seen[key] = max(self.m_seen.get(key, 0), int(M))
            if len(self.m_seen) > 64:                               # (cameras of many sizes: keep the table small)
                self.m_seen.pop(next(iter(self.m_seen)))
        self.capacity = max(self.capacity, int(M * self.HEADROOM) + 4096)

    def overflowed(self, need: int, key=None) -> int:
        """An asynchronous or graphed frame needed ``need`` entries: it rendered empty and the optimiser launches behind it
        did nothing (skip_flag).  Clear the word (stream-ordered behind those launches), make room and have the call that
        follows read M back.  Returns the capacity that was too small."""
        self.status.zero_()
        self.overflows += 1
        self.force_sync = True
        old = self.capacity
        self.saw(key, need)
        return old

    def watchdog_fired(self, message: str):
        self.status.zero_()
        raise L.QedSplatError(message)

    def read_words(self):
        """[M of the last binning call, overflow, watchdog] by one synchronous copy."""
        return self.words[:3].tolist()

    def skip_flag_ptr(self) -> int:
        """Device address of the overflow word: what the optimiser launches take as ``skip_flag``."""
        return self.overflow_word.data_ptr()

    def arm_pending(self, words, key) -> None:
        """An asynchronous frame has been enqueued whose {M, overflow} will land in ``words``: the next call looks."""
        self.frame += 1
        self.pending = (words, key, self.frame)

    def counted_step(self, opt) -> None:
        """An optimiser with a host step counter has counted a step whose launch sits behind the current frame (and takes
        its overflow word as skip_flag): if that frame turns out to have overflowed, THAT optimiser takes the step back --
        not every optimiser of the device (another model's, one that did not step this iteration)."""
        opt.__dict__["_qed_frame"] = self.frame

    def take_overflow_flag(self) -> bool:
        """Did an asynchronous frame overflow since this was last asked?  (get_outputs puts it into ``info``.)"""
        flag, self.last_overflow = self.last_overflow, False
        return flag

    def poll_pending(self) -> None:
        if self.pending is None:
            return
        words, key, frame = self.pending
        self.pending = None
        if words[0] < 0:
            # the host is a frame ahead of the device: wait for that frame's binning.  A few looks back to back (the word
            # usually lands within microseconds), then sleeps that double up to 100 us: a host that runs ahead of a ~1 ms
            # step does not burn a core on it, and wakes at most a tenth of a step late
            t_wait = time.monotonic()
            deadline = t_wait + self.POLL_TIMEOUT_S
            looks, nap = 0, 5e-6
            while words[0] < 0:
                looks += 1
                if looks <= 8:
                    time.sleep(0)
                    continue
                time.sleep(nap)
                nap = min(2.0 * nap, 1e-4)
                if time.monotonic() > deadline:
                    torch.cuda.synchronize(self.device)             # surfaces a device fault as its own error
                    if words[0] < 0:
                        # the frame has finished and its words are not here: the store into pinned memory does not reach
                        # this host (a runtime / allocator configuration this was not tested on).  Take the frame's words
                        # from device memory -- nothing has run since -- and read every later count back by copy.
                        words[0], words[1], words[2] = self.read_words()
                        self.host_words_ok = False
                        warnings.warn("qed_splatter_amd: the intersection count did not arrive through pinned host memory; "
                                      "falling back to a synchronous read-back per call", RuntimeWarning, stacklevel=3)
            self.waited_s += time.monotonic() - t_wait
        M, overflow, watchdog = int(words[0]), int(words[1]), int(words[2])
        if watchdog:
            self.watchdog_fired("the radix-sort look-back watchdog fired in the previous asynchronous rasterization: "
                                "that frame's list was mis-sorted")
        if overflow:
            old = self.overflowed(overflow, key)
            self.last_overflow = True
            for opt in list(self.steppers):                        # (the host is at most one frame ahead: ONE step was skipped)
                if opt.__dict__.get("_qed_frame") == frame:        # ... by the optimisers that stepped behind THAT frame
                    opt.__dict__["_qed_frame"] = None
                    opt.on_skipped_step()
            warnings.warn(f"qed_splatter_amd: an asynchronous rasterization needed {overflow} tile intersections, more "
                          f"than the buffer held ({old}); that frame rendered empty and its optimiser step was skipped "
                          f"on the device.  Capacity raised to {self.capacity}.", RuntimeWarning, stacklevel=3)
            return
        self.saw(key, M)


_WORKSPACES: Dict[int, _Workspace] = {}


def _workspace(device) -> _Workspace:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ws = _WORKSPACES.get(idx)
    if ws is None:
        ws = _WORKSPACES[idx] = _Workspace(torch.device("cuda", idx))
    return ws


def _bin_and_sort(N, C, means2d, radii, depths, tiles_per_gauss, block_sums, tile_w, tile_h, sync=True, splats=None,
                  size=None, tile_masks=None, capture_slot=None):
    """Tile binning (qed_bin_tiles): one C call that leaves the list sorted by (camera, tile, depth) and the tile
    offsets.

    Returns (isect_ids, flatten_ids, offsets, M).  With ``sync=False`` -- honoured only for a shape
    ``(width, height, N, C)`` whose capacity has been calibrated by a synchronous call (_Workspace) -- nothing is read
    back: M and isect_ids are None and flatten_ids keeps its capacity length.
    ``capture_slot`` (while a hipGraph is being captured): the pinned (words, address) pair every REPLAY of the captured
    launch stores {M, overflow, watchdog} into -- the replaying code sets words[0] = -1 before a replay and hands the pair
    to ``_Workspace.arm_pending`` after it (segments.OutputsSegment), exactly as an eager asynchronous call does.
    """
    lib = L.load()
    dev = means2d.device
    ws = _workspace(dev)
    n_tiles = tile_w * tile_h
    key = (tuple(size) if size is not None else (tile_w, tile_h), N, C)
    n_isect = ws.n_isect               # (read by the kernels of this call only; launches are stream-ordered)
    offsets = torch.empty(C * n_tiles + 1, dtype=torch.int32, device=dev)
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing:
        # inside a hipGraph capture nothing may touch the host: capacity is frozen at its calibrated value
        if not ws.may_capture(key):
            raise L.QedSplatError("run one eager call of this shape (image size, number of Gaussians, cameras) before "
                                  "capturing: it calibrates the intersection capacity")
        sync = False
    else:
        ws.poll_pending()
        if not ws.may_skip_readback(key):
            sync = True                                   # first call of a shape, or the call after an overflow
    if ws.capacity == 0:
        ws.capacity = max(1 << 16, 8 * C * N)
    # which pipeline (both give the same list bit for bit): by the longest list this shape has produced, not by the
    # (generously padded) capacity the library's own QED_BIN_AUTO would go by
    mode = L.bin_mode()
    if mode == L.BIN_AUTO and ws.m_seen.get(key, 0) > 0:
        mode = L.BIN_BUCKET if int(1.25 * ws.m_seen[key]) <= 1024 * C * n_tiles else L.BIN_TWO_STAGE
    host = host_ptr = None
    if not sync and not capturing:
        host, host_ptr = ws.host_slot()
    elif capturing and capture_slot is not None:
        host, host_ptr = capture_slot
    for _attempt in range(2):
        cap = ws.capacity
        flatten_ids = torch.empty(cap, dtype=torch.int32, device=dev)
        isect_ids = torch.empty(cap, dtype=torch.int64, device=dev) if sync else None
        scratch = torch.empty(int(lib.qed_bin_workspace_bytes(C * N, cap)), dtype=torch.uint8, device=dev)
        L.check(lib.qed_bin_tiles(N, C, L.ptr(means2d), L.ptr(radii), L.ptr(depths), L.ptr(tiles_per_gauss), L.ptr(splats),
                                  L.ptr(tile_masks), L.ptr(block_sums), tile_w, tile_h, cap, mode, L.ptr(flatten_ids), L.ptr(offsets),
                                  L.ptr(n_isect), L.ptr(isect_ids), L.ptr(scratch), scratch.numel(), L.ptr(ws.status),
                                  host_ptr, L.current_stream()), "qed_bin_tiles")
        if capturing:
            return None, flatten_ids, offsets, None
        if not sync:
            ws.arm_pending(host, key)
            return None, flatten_ids, offsets, None
        # one host read: M, the overflow word and the look-back watchdog word
        M, overflow, watchdog = ws.read_words()
        if watchdog:
            ws.watchdog_fired("the radix-sort look-back watchdog fired: the list of this frame is mis-sorted")
        if overflow == 0:
            ws.saw(key, M)
            ws.force_sync = False
            return isect_ids[:M], flatten_ids[:M], offsets, M
        # (this very call renders again below: no frame was lost, so no overflow is counted and nobody is told)
        ws.status.zero_()
        ws.saw(key, overflow)
    raise L.QedSplatError("intersection buffer overflow persisted after regrowth")
