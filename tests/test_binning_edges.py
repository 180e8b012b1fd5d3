"""qed_bin_tiles on the crafted inputs of tests/binning_cases.py: key widths of one to four radix passes, power-of-two
tile counts, unused camera codes, rectangles up to and beyond 1 023 tiles wide, per-wave totals on both sides of 4 096,
the packed-count marker, runs on both sides of 512 and 2 048 under six depth patterns, and capacities of M and M - 1.
Every pipeline, with and without isect_ids, bit for bit against the oracle; tests/test_binning_edges_cpu.py holds each
case to the branch it is named after.  Run with `pytest -m gpu` on an MI355X."""
from __future__ import annotations

import ctypes

import pytest
import torch

from tests import binning_cases as B

pytestmark = pytest.mark.gpu

GUARD = 1024
SENTINEL = -7
MODES = {"two_stage": 1, "tile_sort": 2, "bucket": 3}          # _lib.BIN_TWO_STAGE, BIN_TILE_SORT, BIN_BUCKET

_DEV = {}


def _inputs(c, dev):
    """The case's inputs on the device, uploaded once."""
    if c.name not in _DEV:
        _DEV[c.name] = tuple(t.to(dev).contiguous() for t in (c.means2d, c.radii, c.depths, c.tiles_per_gauss))
    return _DEV[c.name]


def _bin(lib, dev, c, mode, with_ids, capacity, culled=False):
    """One call of qed_bin_tiles without splat records, tile masks or block sums.  -> dict of host tensors."""
    from qed_splatter_amd import _lib as L
    assert (L.BIN_TWO_STAGE, L.BIN_TILE_SORT, L.BIN_BUCKET) == tuple(MODES.values())
    means2d, radii, depths, tpg = _inputs(c, dev)
    if culled:
        radii, tpg = torch.zeros_like(radii), torch.zeros_like(tpg)
    S, n_tot = c.C * c.N, c.C * c.tile_w * c.tile_h
    flat = torch.full((capacity + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    ids = torch.full((capacity + GUARD,), SENTINEL, dtype=torch.int64, device=dev) if with_ids else None
    offsets = torch.full((n_tot + 1,), SENTINEL, dtype=torch.int32, device=dev)
    n_isect = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.qed_bin_workspace_bytes(S, capacity))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    host = torch.full((4,), -1, dtype=torch.int32).pin_memory()
    dptr = ctypes.c_void_p()
    assert lib.qed_host_device_pointer(host.data_ptr(), ctypes.addressof(dptr)) == 0
    rc = lib.qed_bin_tiles(c.N, c.C, L.ptr(means2d), L.ptr(radii), L.ptr(depths), L.ptr(tpg), 0, 0, 0, c.tile_w, c.tile_h,
                           capacity, mode, L.ptr(flat), L.ptr(offsets), L.ptr(n_isect), L.ptr(ids), L.ptr(ws), ws.numel(),
                           L.ptr(status), dptr.value, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.qed_last_error()
    torch.cuda.synchronize()
    return dict(flat=flat.cpu(), ids=None if ids is None else ids.cpu(), offsets=offsets.cpu(), n_isect=int(n_isect),
                status=status.cpu().tolist(), host=host.tolist())


def _guard_untouched(out, capacity):
    assert bool((out["flat"][capacity:] == SENTINEL).all()), "flatten_ids written past the capacity"
    if out["ids"] is not None:
        assert bool((out["ids"][capacity:] == SENTINEL).all()), "isect_ids written past the capacity"


def _check_list(c, out, capacity):
    M = c.M
    assert out["n_isect"] == M
    assert out["status"] == [0, 0, 0, 0]
    assert out["host"] == [M, 0, 0, 0]
    assert torch.equal(out["offsets"][:-1], c.offsets.reshape(-1)) and int(out["offsets"][-1]) == M
    assert torch.equal(out["flat"][:M], c.flatten_ids)
    if out["ids"] is not None:
        assert torch.equal(out["ids"][:M], c.keys)
    _guard_untouched(out, capacity)


def _both(lib, dev, c, mode, capacity, **kw):
    """With isect_ids and with a null isect_ids: the same outputs."""
    a = _bin(lib, dev, c, mode, True, capacity, **kw)
    b = _bin(lib, dev, c, mode, False, capacity, **kw)
    assert a["n_isect"] == b["n_isect"] and a["status"] == b["status"] and a["host"] == b["host"]
    assert torch.equal(a["offsets"], b["offsets"])
    n = a["n_isect"]
    assert torch.equal(a["flat"][:n], b["flat"][:n]) and torch.equal(a["flat"][capacity:], b["flat"][capacity:])
    return a, b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", B.NAMES)
def test_list_equals_oracle(cuda, lib, name, mode):
    """capacity == M throughout: `all > capacity` must not fire at equality.  A bucket request on a key wider than 16
    bits is served by the tile-sort pipeline and gives the same list."""
    c = B.case(name)
    assert c.M > 0
    for out in _both(lib, cuda, c, MODES[mode], c.M):
        _check_list(c, out, c.M)


CAPACITY_CASES = ("kw_16x16x1", "kw_128x128x3")          # 9 key bits (the bucket pipeline itself) and 17 (its fallback)


@pytest.mark.parametrize("name", CAPACITY_CASES)
def test_capacity_one_short(cuda, lib, name):
    """capacity == M - 1: status[0] = M, n_isect = 0, host words [0, M, 0, 0], nothing past the capacity; offsets and
    guard the same in the three pipelines."""
    c = B.case(name)
    cap = c.M - 1
    outs = {}
    for mode, m in MODES.items():
        for out in _both(lib, cuda, c, m, cap):
            assert out["status"] == [c.M, 0, 0, 0] and out["n_isect"] == 0 and out["host"] == [0, c.M, 0, 0], mode
            _guard_untouched(out, cap)
        outs[mode] = out
    for mode in ("tile_sort", "bucket"):
        assert torch.equal(outs[mode]["offsets"], outs["two_stage"]["offsets"]), mode
        assert torch.equal(outs[mode]["flat"][cap:], outs["two_stage"]["flat"][cap:]), mode
    assert int(outs["two_stage"]["offsets"].abs().max()) == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CAPACITY_CASES)
def test_every_slot_culled(cuda, lib, name, mode):
    """M == 0 with S > 0 (all radii zero): zero offsets, n_isect = 0, zero host words, status clear."""
    c = B.case(name)
    for out in _both(lib, cuda, c, MODES[mode], c.M, culled=True):
        assert out["n_isect"] == 0 and out["status"] == [0, 0, 0, 0] and out["host"] == [0, 0, 0, 0]
        assert int(out["offsets"].abs().max()) == 0
        _guard_untouched(out, c.M)
