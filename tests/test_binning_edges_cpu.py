"""The crafted binning cases (tests/binning_cases.py) reach what their names say, the oracle they are compared with
agrees with a per-entry restatement of the list, and qed_bin_tiles refuses a key wider than 32 bits on the host.  No
GPU needed."""
from __future__ import annotations

import ctypes as C
from collections import Counter

import numpy as np
import pytest
import torch

from tests import binning_cases as B


@pytest.mark.parametrize("name", B.NAMES)
def test_case_reaches_what_its_name_claims(name):
    """A condition on the inputs, not a measurement: if a case drifts off its branch the GPU tests of it prove nothing."""
    c = B.case(name)
    s = B.census(c)
    assert B.CLAIMS[name], name
    for what, want in B.CLAIMS[name].items():
        got = s[what]
        if isinstance(want, tuple):
            assert want[0] <= got <= want[1], (name, what, got, want)
        else:
            assert got == want and type(got) is type(want), (name, what, got, want)
    # the census agrees with itself and with the list
    assert s["passes"] == (s["end_bit"] + 7) // 8 and s["end_bit"] <= 32
    assert sum(k * v for k, v in s["run_lengths"].items()) == c.M == int(c.tiles_per_gauss.sum())
    assert c.offsets.shape == (c.C, c.tile_h, c.tile_w) and c.flatten_ids.dtype == torch.int32
    if c.M:
        assert 0 <= int(c.flatten_ids.min()) and int(c.flatten_ids.max()) < c.C * c.N


def test_branches_are_covered_between_the_cases():
    """Every pass count, both parities of the buffer deal, both sides of each threshold."""
    cs = {n: B.census(B.case(n)) for n in B.NAMES}
    assert {s["passes"] for s in cs.values()} == {1, 2, 3, 4}
    assert {s["end_bit"] for s in cs.values()} >= {7, 8, 9, 17, 20, 24, 25}
    # both sides of the bucket pipeline's 16-bit limit, and unused camera codes on both sides
    assert {16, 17} <= {s["end_bit"] for s in cs.values()}
    assert any(s["end_bit"] <= 16 and s["unused_cam_codes"] > 0 for s in cs.values())
    assert any(s["end_bit"] > 16 and s["unused_cam_codes"] > 0 for s in cs.values())
    assert cs["wave_4096"]["waves_by_search"] == 0 and cs["wave_4097"]["waves_by_search"] == 1
    assert cs["wave_4096"]["max_wave_total"] == B.WAVE_BITS_MAX
    assert cs["wide_3000"]["max_width"] > 1023 == cs["marker"]["max_width"]
    assert any(s["marker_reached"] for s in cs.values()) and not cs["full_256x256"]["marker_reached"]
    runs = cs["runs_random"]["run_lengths"]
    for edge in (B.TILE_WAVE_ITEMS, B.TILE_SORT_ITEMS):
        assert runs[edge] == 1 and runs[edge + 1] == 1 and runs[edge - 1] == 1
    # the same slots under every depth pattern: only the depths differ
    for p in B.DEPTH_PATTERNS:
        a, b = B.case("runs_equal"), B.case(f"runs_{p}")
        assert torch.equal(a.means2d, b.means2d) and torch.equal(a.radii, b.radii)
        assert torch.equal(a.tiles_per_gauss, b.tiles_per_gauss) and torch.equal(a.offsets, b.offsets)
    assert Counter(B.RUN_COUNTS) == runs


def _restated(c):
    """The list, entry by entry: rectangle in float32 scalars, one key per tile in row-major order, a stable sort, the
    offsets by counting."""
    f = np.float32
    tile_bits, _ = B.key_bits(c)
    T = c.tile_w * c.tile_h
    entries, tpg = [], []
    means, radii, depth_bits = c.means2d.numpy(), c.radii.numpy(), c.depths.numpy().view(np.uint32)
    for cam in range(c.C):
        for n in range(c.N):
            r = int(radii[cam, n])
            if r <= 0:
                tpg.append(0)
                continue
            tx, ty, tr = means[cam, n, 0] / f(16), means[cam, n, 1] / f(16), f(r) / f(16)
            clamp = lambda v, hi: min(max(0, int(v)), hi)
            x0, x1 = clamp(np.floor(f(tx - tr)), c.tile_w), clamp(np.ceil(f(tx + tr)), c.tile_w)
            y0, y1 = clamp(np.floor(f(ty - tr)), c.tile_h), clamp(np.ceil(f(ty + tr)), c.tile_h)
            tpg.append((x1 - x0) * (y1 - y0))
            dbits = int(depth_bits[cam, n])
            for y in range(y0, y1):
                for x in range(x0, x1):
                    entries.append(((((cam << tile_bits) | (y * c.tile_w + x)) << 32) | dbits, cam * c.N + n))
    entries.sort(key=lambda e: e[0])                          # (Python's sort is stable)
    offsets, i = [], 0
    for cam in range(c.C):
        for t in range(T):
            while i < len(entries) and ((entries[i][0] >> 32) >> tile_bits, (entries[i][0] >> 32) & ((1 << tile_bits) - 1)) < (cam, t):
                i += 1
            offsets.append(i)
    return tpg, [e[0] for e in entries], [e[1] for e in entries], offsets


@pytest.mark.parametrize("name", ["borders", "kw_17x15x1"])
def test_oracle_against_a_per_entry_restatement(name):
    c = B.case(name)
    tpg, keys, fids, offsets = _restated(c)
    assert c.tiles_per_gauss.reshape(-1).tolist() == tpg
    assert c.keys.tolist() == keys and c.flatten_ids.tolist() == fids and c.M == len(keys) > 0
    assert c.offsets.reshape(-1).tolist() == offsets


def test_key_wider_than_32_bits_is_refused_on_the_host(lib):
    """65 536 x 32 768 tiles are 32 tile bits, two cameras one more: refused before any launch, and the message names
    the key width.  Dummy non-null host buffers: nothing is dereferenced on the way to the refusal."""
    buf = (C.c_int32 * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(tile_w, tile_h, n_cam):
        return lib.qed_bin_tiles(10, n_cam, p, p, p, p, 0, 0, 0, tile_w, tile_h, 100, 0, p, p, p, 0, p, 1 << 40, p, 0, 0)
    assert call(65536, 32768, 2) == -1
    err = lib.qed_last_error()
    assert b"qed_bin_tiles" in err and b"key" in err and b"32 bits" in err
    assert call(32768, 32768, 5) == -1 and b"32 bits" in lib.qed_last_error()            # 31 + 3
    # one bit less passes this check and stops at the next one (the workspace), still without a launch
    buf2 = (C.c_int32 * 64)()
    rc = lib.qed_bin_tiles(10, 1, p, p, p, p, 0, 0, 0, 65536, 32768, 100, 0, p, p, p, 0, C.cast(buf2, C.c_void_p), 256,
                           p, 0, 0)
    assert rc == -2 and b"workspace too small" in lib.qed_last_error()
