"""The crafted compositing cases (tests/composite_cases.py) reach what their names say, their decisions stay clear of
the alpha and transmittance thresholds in float64, and the census they are judged by agrees with the oracle's images.
No GPU needed."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import composite_cases as K

MARGIN = 1e-5                     # tests/test_gpu_parity.py: decisions closer than this to a threshold may flip in float32


@pytest.mark.parametrize("name", K.NAMES)
def test_case_reaches_what_its_name_claims(name):
    """A condition on the inputs, not a measurement: if a case drifts off its branch the GPU tests of it prove nothing."""
    c = K.case(name)
    cen = K.census(c)
    assert K.CLAIMS[name], name
    assert K.broken_claims(name, K.figures(c, cen)) == []
    # the lists are well formed: offsets rise to M, every id names a Gaussian of the tile's own camera
    offs = K.tile_runs(c)
    T = c.tile_w * c.tile_h
    assert offs.size == c.C * T + 1 and offs[0] == 0 and offs[-1] == c.M and bool((np.diff(offs) >= 0).all())
    assert c.flatten_ids.dtype == torch.int32 and c.offsets.dtype == torch.int32 and c.flatten_ids.numel() == c.M
    assert c.w <= 64 and c.h <= 48 and c.tile_w == (c.w + 15) // 16 and c.tile_h == (c.h + 15) // 16
    cam_of_entry = np.repeat(np.arange(c.C * T) // T, np.diff(offs))
    assert bool((c.flatten_ids.numpy() // max(c.N, 1) == cam_of_entry).all())


@pytest.mark.parametrize("name", K.NAMES)
def test_decisions_stay_clear_of_their_thresholds(name):
    """At least 99 % of the in-image pixels have every alpha / transmittance decision further than MARGIN from its cut:
    a condition on the inputs, so that the GPU comparison is over (nearly) the whole image."""
    c = K.case(name)
    assert c.margin.shape == (c.C, c.h, c.w)
    assert float((c.margin > MARGIN).double().mean()) >= 0.99


@pytest.mark.parametrize("name", K.NAMES)
def test_census_agrees_with_the_oracle_images(name):
    """The census walks the lists on its own: its last ids and final transmittances are the oracle's."""
    c = K.case(name)
    T = c.tile_w * c.tile_h
    for d in K.census(c):
        cam, (ty, tx) = d["tile"] // T, divmod(d["tile"] % T, c.tile_w)
        sl = (cam, slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
        if d["length"] == 0:
            assert int(c.last_ids[sl].abs().max()) == 0 and float(c.alpha[sl].abs().max()) == 0.0
            assert float(c.render[sl].abs().max()) == 0.0 and bool(torch.isinf(c.margin[sl]).all())
            continue
        assert np.array_equal(d["last_ids"], c.last_ids[sl].reshape(-1).numpy())
        assert d["t_final_min"] == pytest.approx(1.0 - float(c.alpha[sl].max()), rel=1e-9, abs=1e-15)
        assert d["touch"].shape == (d["length"], 4) and d["start"] + d["length"] <= c.M


def test_branches_are_covered_between_the_cases():
    """Every list length beside a batch seam, empty tiles at offset 0, inside the list and at its end, batches with no
    survivor, quadrants that finish in different batches, a stop on either side of the first seam, both per-pixel forms."""
    fs = {n: K.figures(K.case(n), K.census(K.case(n))) for n in K.NAMES}
    assert set(K.SEAM_LENGTHS) == {k * 64 + d for k in (0, 1, 2, 3) for d in (-1, 0, 1) if k * 64 + d > 0} | {2, 257}
    assert fs["empty_leading"]["empty_starts"][0] == 0 < fs["empty_interior"]["empty_starts"][0]
    assert fs["empty_trailing"]["empty_starts"][-1] == fs["empty_trailing"]["M"]
    for n in ("culled_batches_lane0", "culled_batches_lane63"):
        assert len(fs[n]["near_lanes"][0]) % 2 == 1 and fs[n]["near_lanes"][1] == ()
    assert len(set(fs["quadrant_endings"]["quad_last_batch"])) == 3
    assert fs["stop_at_63"]["quad_last_batch"] == (0,) * 4 and fs["stop_at_64"]["quad_last_batch"] == (1,) * 4
    assert {f["n_slow"] for f in fs.values()} == {0, 3}
    assert any(0 < q < 4 for n in K.NAMES if n.startswith("partial_") for q in fs[n]["outside_quadrants"])
    two = K.case("two_cameras")
    assert two.C == 2 and int(two.flatten_ids.max()) >= two.N            # camera 1 names its own copies
