"""Crafted inputs of ``qed_bin_tiles`` and a census of what each of them reaches (tests/test_binning_edges*.py).

Every other binning test goes through ``rasterization()`` on a random scene and so sees the key widths, rectangles and
run lengths that scene happens to have.  ``qed_bin_tiles`` takes ``means2d``, ``radii``, ``depths`` and
``tiles_per_gauss`` directly, so here they are written down on purpose:

* coordinates are integers plus 0.5 and radii are integers, so ``(x +- r) / 16`` is a multiple of 1/32 that is never an
  integer: it is exact in float32 and no floor or ceil sits on a rounding edge;
* depths are positive float32 (some cases build them from their bit patterns: one ulp apart, denormal);
* everything is seeded by the case's name.

``case(name)`` returns the inputs and, from the oracle, ``tiles_per_gauss``, the sorted 64-bit keys, ``flatten_ids``,
the offsets and ``M``.  ``census(case)`` says which branch of the binning the case takes: key width and radix passes,
power-of-two tile count, largest rectangle, per-wave entry totals, the packed-count marker of the two-stage pipeline,
the run lengths and the occupancy of the per-tile sort's 9-bit depth buckets.  ``CLAIMS[name]`` is what the name
promises; tests/test_binning_edges_cpu.py holds every case to it, so the GPU tests cannot drift off their branch.
Pure data and oracle calls: no kernel is touched."""
from __future__ import annotations

import functools
import zlib
from collections import Counter
from types import SimpleNamespace
from typing import Callable, Dict, Tuple

import numpy as np
import torch

from oracle import splat_oracle as O

TILE = 16
WAVE_BITS_MAX = 64 * 64          # isect_emit_kernel: popcount over range-start bits up to here, binary search beyond
TILE_WAVE_ITEMS = 512            # tile_depth_sort_kernel: one wave sorts runs up to here ...
TILE_SORT_ITEMS = 2048           # ... one workgroup in LDS up to here, through global scratch beyond
TILE_BUCKETS = 512
TILE_BUCKET_MAX = 12             # a fuller 9-bit bucket sends a short run to the four radix passes
RUN_COUNTS = (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097)
RUN_TILES = (0, 5, 9, 14, 18, 23, 27, 36, 41, 50, 54, 63)       # of the 8 x 8 grid; first and last tile included
DEPTH_PATTERNS = ("equal", "two", "descending", "random", "crowded", "spread")


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def _bits_to_f32(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _centre(t):
    """Pixel coordinate (integer + 0.5) in the middle of tile column / row ``t``."""
    return 16.0 * np.asarray(t, dtype=np.float64) + 8.5


# ---- builders: -> C, N, tile_w, tile_h, means [C,N,2], radii [C,N], depths [C,N] -------------------------------------
def _small_random(name: str, C: int, N: int, tw: int, th: int):
    """Small Gaussians (radius 1..40, some culled) all over the grid and a little beyond; depths from a pool of 2 000
    values, so bit-equal depths meet in one tile."""
    g = _rng(name)
    x = g.integers(-30, tw * TILE + 30, (C, N)) + 0.5
    y = g.integers(-30, th * TILE + 30, (C, N)) + 0.5
    r = g.integers(1, 41, (C, N))
    r[g.random((C, N)) < 0.15] = 0
    d = g.integers(1, 2001, (C, N)) / 16.0
    return C, N, tw, th, np.stack([x, y], -1), r, d


def _key_width(tw: int, th: int, C: int, N: int) -> Callable:
    return lambda name: _small_random(name, C, N, tw, th)


def _with_rows(name: str, C: int, tw: int, th: int, rows, n_small: int):
    """``rows`` of (x, y, radius, depth) in slots 0.. of every camera, then ``n_small`` small random Gaussians."""
    _, _, _, _, m, r, d = _small_random(name, C, len(rows) + n_small, tw, th)
    for i, (x, y, rad, dep) in enumerate(rows):
        m[:, i] = (x, y)
        r[:, i] = rad
        d[:, i] = dep
    return C, len(rows) + n_small, tw, th, m, r, d


def _full_grid(tw: int, th: int, n_full: int, n_small: int) -> Callable:
    """Gaussians whose rectangle is the whole grid (clipped on every side)."""
    rows = [(8.0 * tw + 0.5, 8.0 * th + 0.5, 16 * max(tw, th), 2.0 + i) for i in range(n_full)]
    return lambda name: _with_rows(name, 1, tw, th, rows, n_small)


def _wide_3000(name: str):
    """3000 x 2800 tiles.  One rectangle 3 000 tiles wide and three rows high (its centre far above the grid, so the clip
    leaves rows 0..2), one of 1 501 x 2 and one of 2 501 x 120 on the bottom edge (the reciprocal row/column split of the
    emit kernel at a width and a row count far past its stated bound), and a few small ones."""
    rows = [(24000.5, -23975.5, 24016, 3.0), (24000.5, 2800 * 16 + 11975.5, 12000, 1.5),
            (24000.5, 2680 * 16 + 20008.5, 20000, 2.25)]
    return _with_rows(name, 1, 3000, 2800, rows, 24)


def _borders(name: str):
    """20 x 12 tiles.  Rectangles clipped by each border and each corner, rectangles with radius > 0 that clip to
    nothing (beyond each border and each corner), one culled slot, one interior."""
    tw, th = 20, 12
    W, H = tw * TILE, th * TILE
    rows = []
    for x, y in ((-10.5, 90.5), (W + 9.5, 90.5), (150.5, -10.5), (150.5, H + 9.5),          # the four borders
                 (-10.5, -10.5), (W + 9.5, -10.5), (-10.5, H + 9.5), (W + 9.5, H + 9.5)):    # the four corners
        rows.append((x, y, 40, 2.0))
    for x, y in ((-100.5, 90.5), (W + 100.5, 90.5), (150.5, -100.5), (150.5, H + 100.5),
                 (-100.5, -100.5), (W + 100.5, H + 100.5)):                                  # radius > 0, no tile
        rows.append((x, y, 20, 1.0))
    rows.append((100.5, 100.5, 0, 1.0))
    rows.append((100.5, 100.5, 30, 0.5))
    return _with_rows(name, 1, tw, th, rows, 0)


def _wave(sizes) -> Callable:
    """40 x 40 tiles; slots 0..63 (one wave of the emit kernel) hold rectangles of the given tile extents, slots 64..
    small random Gaussians.  Depths rise with the slot, so the depth order of the two-stage pipeline is the slot order
    and its waves are the same."""
    rad = {8: 56, 9: 64, 10: 72, 11: 80}          # centre on 16 k + 8.5: radius -> tiles across
    def build(name):
        g = _rng(name)
        C, N, tw, th, m, r, d = _small_random(name, 1, 64 + 150, 40, 40)
        assert len(sizes) == 64
        for i, s in enumerate(sizes):
            if s == "8x6":                        # an 8 x 8 rectangle with two rows above the grid
                m[0, i] = (_centre(g.integers(6, 34)), _centre(1))
                r[0, i] = rad[8]
            else:
                m[0, i] = (_centre(g.integers(6, 34)), _centre(g.integers(6, 34)))
                r[0, i] = rad[s]
        d[0] = 1.0 + np.arange(N) / 64.0
        return C, N, tw, th, m, r, d
    return build


def _marker(name: str):
    """40 000 slots on the 1023 x 65 grid: slot_bits = 16, so a tile count of 65 535 or more does not fit beside the
    slot and goes through the marker.  Two full-grid Gaussians (66 495 tiles each) far apart in the slots, a handful of
    small ones, everything else culled."""
    tw, th, N = 1023, 65, 40000
    C, _, _, _, m, r, d = _small_random(name, 1, N, tw, th)
    keep = _rng(name + "/keep").choice(N, 12, replace=False)
    small = r[0, keep].copy()
    r[:] = 0
    r[0, keep] = np.maximum(small, 1)
    for slot, dep in ((777, 7.0), (39001, 0.25)):
        m[0, slot] = (8.0 * tw + 0.5, 8.0 * th + 0.5)
        r[0, slot] = 16 * tw
        d[0, slot] = dep
    return C, N, tw, th, m, r, d


def _run_depths(pattern: str, g: np.random.Generator, tile_of: np.ndarray) -> np.ndarray:
    n = tile_of.size
    if pattern == "equal":
        return np.full(n, 2.5, np.float32)
    if pattern == "two":
        return np.where(g.random(n) < 0.5, 1.0, 3.0).astype(np.float32)
    if pattern == "descending":                   # distinct, falling with the slot: every run arrives reversed
        return (1.0 + (n - np.arange(n)) / 1024.0).astype(np.float32)
    if pattern == "random":                       # distinct, uniform in the BITS (the buckets are cut in the bits)
        return _bits_to_f32(0x3F800000 + g.choice(1 << 24, n, replace=False))
    if pattern == "crowded":                      # a ladder of 17 depths one ulp apart (with ties), one outlier per run
        d = _bits_to_f32(0x3F800000 + g.integers(0, 17, n))
        for t in np.unique(tile_of[tile_of >= 0]):
            members = np.flatnonzero(tile_of == t)
            d[g.choice(members)] = 1e6
        return d
    if pattern == "spread":                       # sixty orders of magnitude, denormals among them
        d = (10.0 ** g.uniform(-30.0, 30.0, n)).astype(np.float32)
        d[g.choice(n, 40, replace=False)] = _bits_to_f32(g.integers(1, 1 << 23, 40))
        d[g.choice(n, 3, replace=False)] = _bits_to_f32([1, 1, 0x007FFFFF])
        return d
    raise KeyError(pattern)


def _runs(pattern: str) -> Callable:
    """8 x 8 tiles, twelve of them with exactly RUN_COUNTS Gaussians of one tile each (tile centre, radius 1), dealt over
    the slots at random, plus 100 culled slots."""
    def build(name):
        g = _rng("runs")                          # the same slots under every depth pattern
        tile_of = np.concatenate([np.repeat(RUN_TILES, RUN_COUNTS), np.full(100, -1)])
        tile_of = tile_of[g.permutation(tile_of.size)]
        N = tile_of.size
        t = np.maximum(tile_of, 0)
        m = np.stack([_centre(t % 8), _centre(t // 8)], -1)[None]
        r = (tile_of >= 0).astype(np.int64)[None]
        d = _run_depths(pattern, _rng(name), tile_of)[None]
        return 1, N, 8, 8, m, r, d
    return build


_BUILDERS: Dict[str, Callable] = {
    # key widths (tile_w, tile_h, C)
    "kw_17x15x1": _key_width(17, 15, 1, 300),
    "kw_16x16x1": _key_width(16, 16, 1, 300),
    "kw_128x128x3": _key_width(128, 128, 3, 301),
    "kw_256x256x1": _key_width(256, 256, 1, 300),
    "kw_1023x65x5": _key_width(1023, 65, 5, 299),
    "kw_3000x2800x1": _key_width(3000, 2800, 1, 300),
    "kw_512x128x129": _key_width(512, 128, 129, 97),
    # keys of at most 16 bits, which the bucket pipeline takes itself: unused camera codes there, and its widest key
    "kw_17x15x5": _key_width(17, 15, 5, 299),
    "kw_8x8x129": _key_width(8, 8, 129, 97),
    "kw_128x128x2": _key_width(128, 128, 2, 300),
    # rectangles
    "full_1023x65": _full_grid(1023, 65, 2, 5),
    "full_256x256": _full_grid(256, 256, 1, 5),
    "wide_3000": _wide_3000,
    "borders": _borders,
    "wave_4096": _wave([8] * 64),
    "wave_4097": _wave([8] * 62 + [9, "8x6"]),
    "wave_7744": _wave([11] * 64),
    "marker": _marker,
}
_BUILDERS.update({f"runs_{p}": _runs(p) for p in DEPTH_PATTERNS})
NAMES = tuple(_BUILDERS)

_RUNS = {"run_lengths": Counter(RUN_COUNTS)}
# what each name promises of its census (an int or bool: equal; a (lo, hi) tuple: within; a Counter: equal)
CLAIMS: Dict[str, Dict] = {
    "kw_17x15x1": dict(end_bit=8, passes=1, pow2=False),
    "kw_16x16x1": dict(end_bit=9, passes=2, pow2=True),
    "kw_128x128x3": dict(end_bit=17, passes=3, pow2=True, unused_cam_codes=1),
    "kw_256x256x1": dict(end_bit=17, passes=3, pow2=True),
    "kw_1023x65x5": dict(end_bit=20, passes=3, pow2=False, unused_cam_codes=3),
    "kw_3000x2800x1": dict(end_bit=24, passes=3, pow2=False),
    "kw_512x128x129": dict(end_bit=25, passes=4, pow2=True, unused_cam_codes=127),
    "kw_17x15x5": dict(end_bit=11, passes=2, pow2=False, unused_cam_codes=3),
    "kw_8x8x129": dict(end_bit=15, passes=2, pow2=True, unused_cam_codes=127),
    "kw_128x128x2": dict(end_bit=16, passes=2, pow2=True, unused_cam_codes=0),
    "full_1023x65": dict(end_bit=17, max_width=1023, max_tiles=66495, max_wave_total=(2 * 66495, 2 * 66495 + 200)),
    "full_256x256": dict(end_bit=17, pow2=True, max_width=256, max_tiles=65536),
    "wide_3000": dict(end_bit=24, passes=3, max_width=3000, max_tiles=2501 * 120),
    "borders": dict(n_visible_without_tiles=6, min_x0=0, min_y0=0, max_x1=20, max_y1=12),
    "wave_4096": dict(first_wave_total=4096, first_wave_total_depth_order=4096),
    "wave_4097": dict(first_wave_total=4097, first_wave_total_depth_order=4097),
    "wave_7744": dict(first_wave_total=7744, first_wave_total_depth_order=7744),
    "marker": dict(slot_bits=16, marker=65535, marker_reached=True, max_tiles=66495, max_width=1023),
    "runs_equal": dict(_RUNS, n_single_depth_runs=11),
    "runs_two": dict(_RUNS),
    "runs_descending": dict(_RUNS),
    "runs_random": dict(_RUNS, max_bucket_occupancy=(1, TILE_BUCKET_MAX), n_single_depth_runs=0),
    "runs_crowded": dict(_RUNS, max_bucket_occupancy=(TILE_BUCKET_MAX + 1, TILE_WAVE_ITEMS)),
    "runs_spread": dict(_RUNS, max_bucket_occupancy=(1, TILE_BUCKET_MAX), depth_bits_min=1,
                        depth_decades=(59.0, 80.0)),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> SimpleNamespace:
    """The inputs of one case and the oracle's list for them.  Cached and shared: treat every tensor as read-only."""
    C, N, tw, th, m, r, d = _BUILDERS[name](name)
    means2d = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).reshape(C, N, 2)
    radii = torch.from_numpy(np.ascontiguousarray(r, dtype=np.int32)).reshape(C, N)
    depths = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).reshape(C, N)
    frac = means2d.double() - torch.floor(means2d.double())
    assert bool((frac == 0.5).all()) and bool((depths > 0).all()) and bool((radii >= 0).all())
    tpg, keys, fids = O.isect_tiles(means2d, radii, depths, TILE, tw, th)
    offsets = O.isect_offset_encode(keys, C, tw, th)
    return SimpleNamespace(name=name, C=C, N=N, tile_w=tw, tile_h=th, means2d=means2d, radii=radii, depths=depths,
                           tiles_per_gauss=tpg, keys=keys, flatten_ids=fids, offsets=offsets, M=int(keys.numel()))


def key_bits(c) -> Tuple[int, int]:
    """(tile_bits, cam_bits) as qed_bin_tiles counts them."""
    tile_bits = 1
    while (1 << tile_bits) <= c.tile_w * c.tile_h:
        tile_bits += 1
    cam_bits = 0
    while (1 << cam_bits) < c.C:
        cam_bits += 1
    return tile_bits, cam_bits


def _wave_totals(counts: np.ndarray) -> np.ndarray:
    pad = (-counts.size) % 64
    return np.concatenate([counts, np.zeros(pad, counts.dtype)]).reshape(-1, 64).sum(1)


def census(c) -> Dict:
    """What the case reaches, from the inputs and the oracle's list alone."""
    T, S = c.tile_w * c.tile_h, c.C * c.N
    tile_bits, cam_bits = key_bits(c)
    end_bit = tile_bits + cam_bits
    x0, y0, x1, y1 = (t.reshape(-1).numpy() for t in O.tile_rects(c.means2d, c.radii, TILE, c.tile_w, c.tile_h))
    tpg = c.tiles_per_gauss.reshape(-1).numpy().astype(np.int64)
    radii = c.radii.reshape(-1).numpy()
    dbits = c.depths.reshape(-1).numpy().view(np.uint32)
    listed = tpg > 0
    # the emit kernel's waves: 64 consecutive slots -- in slot order (tile-sort, bucket) or in depth order (two-stage:
    # stable sort on the depth bits, culled slots last)
    waves = _wave_totals(tpg)
    order = np.argsort(np.where(radii > 0, dbits, 0xFFFFFFFF).astype(np.uint64), kind="stable")
    waves_d = _wave_totals(tpg[order])
    slot_bits = 1
    while (1 << slot_bits) < S:
        slot_bits += 1
    if slot_bits > 28:
        slot_bits = 32
    marker = (1 << (32 - slot_bits)) - 1 if slot_bits < 32 else None
    # runs of the sorted list
    offs = np.concatenate([c.offsets.reshape(-1).numpy().astype(np.int64), [c.M]])
    runs = np.diff(offs)
    nz = np.flatnonzero(runs)
    out = dict(
        end_bit=end_bit, passes=(end_bit + 7) // 8, tile_bits=tile_bits, cam_bits=cam_bits,
        pow2=T & (T - 1) == 0, unused_cam_codes=(1 << cam_bits) - c.C, M=c.M,
        max_tiles=int(tpg.max(initial=0)), max_width=int((x1 - x0)[listed].max(initial=0)),
        min_x0=int(x0[listed].min(initial=c.tile_w)), min_y0=int(y0[listed].min(initial=c.tile_h)),
        max_x1=int(x1[listed].max(initial=0)), max_y1=int(y1[listed].max(initial=0)),
        n_visible_without_tiles=int(((radii > 0) & ~listed).sum()),
        max_wave_total=int(waves.max(initial=0)), first_wave_total=int(waves[0]),
        max_wave_total_depth_order=int(waves_d.max(initial=0)), first_wave_total_depth_order=int(waves_d[0]),
        waves_by_search=int((waves > WAVE_BITS_MAX).sum()),
        slot_bits=slot_bits, marker=marker, marker_reached=marker is not None and int(tpg.max(initial=0)) >= marker,
        run_lengths=Counter(runs[nz].tolist()), max_run=int(runs.max(initial=0)),
        depth_bits_min=int(dbits[listed].min(initial=0xFFFFFFFF)),
    )
    vis_d = c.depths.reshape(-1).numpy()[listed].astype(np.float64)
    out["depth_decades"] = float(np.log10(vis_d.max() / vis_d.min())) if vis_d.size else 0.0
    # tile_sort_wave's 9-bit buckets, with its own float32 formula, over every run of 2..512 entries of several depths
    occupancy, single = 0, 0
    if nz.size:
        key = dbits[c.flatten_ids.numpy()]
        kmin, kmax = np.minimum.reduceat(key, offs[nz]), np.maximum.reduceat(key, offs[nz])
        single = int(((kmin == kmax) & (runs[nz] >= 2)).sum())
        run_of = np.repeat(np.arange(nz.size), runs[nz])
        short = (runs[nz] >= 2) & (runs[nz] <= TILE_WAVE_ITEMS) & (kmin < kmax)
        sel = short[run_of]
        if sel.any():
            span = np.where(kmax > kmin, kmax - kmin, 1).astype(np.uint32)
            scale = (np.float32(511.99) / span.astype(np.float32)).astype(np.float32)
            prod = ((key - kmin[run_of]).astype(np.uint32).astype(np.float32) * scale[run_of]).astype(np.float32)
            bkt = np.minimum(prod[sel].astype(np.int64), TILE_BUCKETS - 1)
            occupancy = int(np.unique(run_of[sel] * TILE_BUCKETS + bkt, return_counts=True)[1].max())
    out["max_bucket_occupancy"] = occupancy
    out["n_single_depth_runs"] = single
    return out


def census_line(name: str) -> str:
    """One line per case for a report: end_bit, passes, largest rectangle, largest wave total, run lengths."""
    c = case(name)
    s = census(c)
    runs = s["run_lengths"]
    shown = dict(sorted(runs.items())) if len(runs) <= 12 else f"{sum(runs.values())} runs, longest {s['max_run']}"
    return (f"{name}: {c.tile_w}x{c.tile_h}x{c.C} N={c.N} M={c.M} end_bit={s['end_bit']} passes={s['passes']} "
            f"pow2={s['pow2']} max_rect={s['max_tiles']} (w={s['max_width']}) max_wave={s['max_wave_total']} "
            f"slot_bits={s['slot_bits']} marker={s['marker']} bucket_occupancy={s['max_bucket_occupancy']} "
            f"run_lengths={shown}")
