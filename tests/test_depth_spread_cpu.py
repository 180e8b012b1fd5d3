"""The reference of the depth-spread tests (tests/depth_spread_cases.py) held to its own claims with the float64 oracle alone,
on the crafted tile lists of tests/composite_cases.py: the closed form A D2 - D^2 is the pairwise sum, every case has pixels
with a spread and -- where a tile lists a single Gaussian -- pixels whose spread is exactly 0, almost no pixel sits on a
threshold, and the thin setting is one where raw float32 moments would cancel.  No kernel is touched."""
from __future__ import annotations

import pytest
import torch

from tests import composite_cases as K
from tests import depth_spread_cases as R

_REF = {}


def _ref(name, setting):
    """Once per (case, setting): closed form, pairwise form and contributor counts on the oracle's own projection."""
    key = (name, setting)
    if key not in _REF:
        c = K.case(name)
        z = c.depths if setting == "projected" else R.thin_depths(c.depths)
        with torch.no_grad():
            closed, A, D, D2 = R.closed_form(c, c.means2d, c.conics, c.opac, z)
        pair, count = R.pairwise(c, c.means2d, c.conics, c.opac, z)
        _REF[key] = (c, closed, A, D2, pair, count)
    return _REF[key]


@pytest.mark.parametrize("setting", R.SETTINGS)
@pytest.mark.parametrize("name", K.NAMES)
def test_closed_form_is_the_pairwise_sum(name, setting):
    """A D2 - D^2 = sum_{i<j} w_i w_j (z_i - z_j)^2.  Bound: the closed form subtracts two numbers of size A D2 <= 17 (thin:
    z <= 4.02, A <= 1) in float64, so it is off by a few 1e-15 at most; 1e-12 absolute is three orders above that and eight
    below the spreads the cases have."""
    c, closed, A, D2, pair, count = _ref(name, setting)
    assert float((closed - pair).abs().max()) <= 1e-12
    assert float(pair.min()) >= 0.0
    # no pair, no spread: exactly, by the pairwise form
    assert bool((pair[count <= 1] == 0).all())
    assert bool((count[A == 0] == 0).all()) and bool((A[count == 0] == 0).all())


@pytest.mark.parametrize("name", K.NAMES)
def test_cases_reach_both_kinds_of_pixel(name):
    """Every case with a list has pixels with spread > 0; a case with a tile that lists one Gaussian has pixels that this
    Gaussian alone reaches, where the spread is exactly 0."""
    c, _, _, _, pair, count = _ref(name, "projected")
    if c.M == 0:
        assert float(pair.max()) == 0.0 and int(count.max()) == 0
        return
    assert bool((pair > 0).any())
    lens = torch.diff(torch.from_numpy(K.tile_runs(c)))
    if bool((lens == 1).any()):
        single = count == 1
        assert bool(single.any())
        assert bool((pair[single] == 0).all())


@pytest.mark.parametrize("name", K.NAMES)
def test_almost_no_pixel_sits_on_a_threshold(name):
    c = K.case(name)
    share = float((c.margin <= R.MARGIN).double().mean())
    print(f"[depth spread] {name}: share of pixels with margin <= {R.MARGIN:g}: {share:.4f}")
    assert share <= R.MAX_UNSAFE_SHARE


@pytest.mark.parametrize("name", [n for n in K.NAMES if n != "empty_all"])
def test_thin_setting_cancels_in_raw_moments(name):
    """At the median covered pixel of the thin setting A D2 exceeds the spread by more than 1e4: float32 raw moments (24 bits)
    would keep at most three digits of it."""
    _, _, A, D2, pair, _ = _ref(name, "thin")
    covered = A > 0
    assert bool(covered.any())
    ratio = (A * D2)[covered] / pair[covered]                 # (inf where one Gaussian contributes)
    assert float(ratio.median()) > 1e4
