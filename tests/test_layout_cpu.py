"""layout.py on the CPU: the flat parameter layout's offsets, shapes, views, the aliasing predicate and the ctypes begins,
and the model that holds one.  No kernel library is needed."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

from qed_splatter_amd.layout import GROUP_ORDER, FlatLayout, group_widths

#           sh_degree -> floats per Gaussian of the six groups
WIDTHS = {0: (3, 3, 4, 1, 3, 0), 1: (3, 3, 4, 1, 3, 9), 2: (3, 3, 4, 1, 3, 24), 3: (3, 3, 4, 1, 3, 45)}
BEGINS_N5 = {0: [0, 15, 30, 50, 55, 70, 70], 1: [0, 15, 30, 50, 55, 70, 115], 2: [0, 15, 30, 50, 55, 70, 190],
             3: [0, 15, 30, 50, 55, 70, 295]}
BEGINS_N1 = {0: [0, 3, 6, 10, 11, 14, 14], 1: [0, 3, 6, 10, 11, 14, 23], 2: [0, 3, 6, 10, 11, 14, 38],
             3: [0, 3, 6, 10, 11, 14, 59]}


def _tensors(n, d, dtype=torch.float32):
    g = torch.Generator().manual_seed(10 * n + d)
    k = (d + 1) ** 2 - 1
    shapes = dict(means=(n, 3), scales=(n, 3), quats=(n, 4), opacities=(n, 1), features_dc=(n, 3), features_rest=(n, k, 3))
    return {name: torch.randn(shapes[name], generator=g).to(dtype) for name in GROUP_ORDER}


@pytest.mark.parametrize("d", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 5])
def test_begins_total_shapes_and_spans_against_literals(n, d):
    assert group_widths(d) == WIDTHS[d]
    lay = FlatLayout.for_sh_degree(n, d)
    want = {0: [0] * 7, 1: BEGINS_N1[d], 5: BEGINS_N5[d]}[n]
    assert lay.n == n and lay.widths == WIDTHS[d] and lay.begin == want and isinstance(lay.begin, list)
    assert lay.total == want[-1] == n * sum(WIDTHS[d])
    k = (d + 1) ** 2 - 1
    assert lay.shapes == ((n, 3), (n, 3), (n, 4), (n, 1), (n, 3), (n, k, 3))
    for g, name in enumerate(GROUP_ORDER):
        assert lay.span(name) == (want[g], want[g + 1])
        assert torch.Size(lay.shapes[g]).numel() == want[g + 1] - want[g]


def test_of_and_resized_keep_the_widths_and_equality_goes_by_n_and_widths():
    for d in (0, 3):
        for n in (0, 5):                                             # (n = 0: the widths still come from the shapes)
            lay = FlatLayout.of(_tensors(n, d))
            assert lay == FlatLayout.for_sh_degree(n, d) and lay.widths == WIDTHS[d]
            assert hash(lay) == hash(FlatLayout.for_sh_degree(n, d))
            big = lay.resized(7)
            assert big.n == 7 and big.widths == WIDTHS[d] and big == FlatLayout.for_sh_degree(7, d)
            assert lay.resized(0).resized(n) == lay
    a = FlatLayout.for_sh_degree(5, 3)
    assert a == FlatLayout(5, WIDTHS[3]) and a != FlatLayout.for_sh_degree(6, 3) and a != FlatLayout.for_sh_degree(5, 2)
    assert a != (5, WIDTHS[3]) and len({a, FlatLayout(5, WIDTHS[3]), a.resized(6)}) == 2
    # an opacity vector [N] and an [N,1] column are the same group
    t = _tensors(5, 3)
    t["opacities"] = t["opacities"].reshape(5)
    assert FlatLayout.of(t) == a


@pytest.mark.parametrize("d", [0, 3])
def test_views_alias_the_flat_buffer_at_the_begins(d):
    lay = FlatLayout.for_sh_degree(5, d)
    flat = lay.empty("cpu")
    assert flat.shape == (lay.total,) and flat.dtype == torch.float32
    flat.copy_(torch.arange(lay.total))
    views = lay.views(flat)
    assert tuple(views) == GROUP_ORDER
    for g, name in enumerate(GROUP_ORDER):
        v = views[name]
        assert tuple(v.shape) == lay.shapes[g] and v.is_contiguous()
        if v.numel():
            assert v.data_ptr() == flat.data_ptr() + 4 * lay.begin[g]
            assert torch.equal(v.reshape(-1), flat[lay.begin[g]:lay.begin[g + 1]])
            v.fill_(-float(g + 1))                                   # a write through the view lands in the flat buffer
            assert bool((flat[lay.begin[g]:lay.begin[g + 1]] == -float(g + 1)).all())
    # a flat buffer that is itself a view at an offset of a larger allocation
    big = torch.zeros(lay.total + 3)
    inner = lay.views(big[3:])
    assert inner["scales"].data_ptr() == big.data_ptr() + 4 * (3 + lay.begin[1])
    params, exp_avg, exp_avg_sq = lay.empty_like_state("cpu")
    assert params.numel() == exp_avg.numel() == exp_avg_sq.numel() == lay.total
    assert len({params.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr()}) == 3


@pytest.mark.parametrize("d", [0, 3])
def test_aliases_is_true_for_the_views_of_its_own_buffer_only(d):
    lay = FlatLayout.for_sh_degree(5, d)
    flat = torch.randn(lay.total)
    views = lay.views(flat)
    if d == 0:
        assert views["features_rest"].numel() == 0 and views["features_rest"].data_ptr() == 0
    six = lambda **other: [other.get(name, views[name]) for name in GROUP_ORDER]                       # noqa: E731
    assert lay.aliases(flat, six())
    assert lay.aliases(flat.data_ptr(), six())                                      # the address in place of the tensor
    assert not lay.aliases(flat, six(quats=views["quats"].clone()))                 # one group is a copy
    assert not lay.aliases(flat, six(means=views["scales"], scales=views["means"]))                   # two swapped
    assert not lay.aliases(flat, six(opacities=views["opacities"].double()))
    assert not lay.aliases(flat.double(), six())
    longer = torch.randn(lay.total + 1)
    assert not lay.aliases(flat[:lay.total - 1], six())                             # the flat buffer one element short
    assert not lay.aliases(longer, list(lay.views(longer[:lay.total]).values()))    # ... and one too long
    assert not lay.resized(4).aliases(flat, six())


def test_ctypes_begins():
    lay = FlatLayout.for_sh_degree(5, 3)
    assert isinstance(lay.c_begin, C.c_int64 * 7) and list(lay.c_begin) == BEGINS_N5[3]
    assert lay.c_begin is lay.c_begin and lay.c_begin_ptr is lay.c_begin_ptr
    assert isinstance(lay.c_begin_ptr, C.c_void_p) and lay.c_begin_ptr.value == C.addressof(lay.c_begin)
    for lo, hi in ((0, lay.total), (16, 48), (lay.total, lay.total)):
        got = lay.clipped_begin(lo, hi)
        assert isinstance(got, C.c_int64 * 7)
        assert list(got) == [min(max(b - lo, 0), hi - lo) for b in BEGINS_N5[3]]
    assert list(lay.clipped_begin(16, 48)) == [0, 0, 14, 32, 32, 32, 32]
    assert list(FlatLayout.for_sh_degree(0, 0).c_begin) == [0] * 7
    # a copy (of a model, say) is rebuilt with an array of its own
    import copy
    twin = copy.deepcopy(lay)
    assert twin == lay and twin.c_begin is not lay.c_begin and list(twin.c_begin) == BEGINS_N5[3]


@pytest.mark.parametrize("d", [0, 3])
def test_model_on_the_cpu_holds_its_layout(d):
    from qed_splatter_amd.model import GROUP_ORDER as FROM_MODEL
    from qed_splatter_amd.model import QEDSplatterModel
    from qed_splatter_amd.seed_init import group_widths as from_seed_init
    assert FROM_MODEL is GROUP_ORDER and from_seed_init is group_widths
    n = 3
    t = _tensors(n, d)
    m = QEDSplatterModel(None, **t)
    assert m.layout == FlatLayout.for_sh_degree(n, d)
    assert m.group_begin == m.layout.begin and isinstance(m.group_begin, list) and m.group_names == list(GROUP_ORDER)
    assert m.layout.aliases(m.flat_params, [m.gauss_params[k] for k in GROUP_ORDER])
    assert all(torch.equal(m.gauss_params[k].detach(), t[k]) for k in GROUP_ORDER)
    shapes = {k: tuple(m.gauss_params[k].shape[1:]) for k in GROUP_ORDER}
    # N = 0 and back: the widths and the per-Gaussian shapes stay
    m.rebind_flat(torch.empty(0), 0)
    assert m.num_points == 0 and m.layout == FlatLayout.for_sh_degree(0, d) and m.group_begin == [0] * 7
    assert {k: tuple(m.gauss_params[k].shape) for k in GROUP_ORDER} == {k: (0,) + s for k, s in shapes.items()}
    flat = torch.arange(float(n * sum(group_widths(d))))
    m.rebind_flat(flat, n)
    assert m.layout == FlatLayout.for_sh_degree(n, d) and m.flat_params is flat
    assert {k: tuple(m.gauss_params[k].shape) for k in GROUP_ORDER} == {k: (n,) + s for k, s in shapes.items()}
    assert m.layout.aliases(flat, [m.gauss_params[k] for k in GROUP_ORDER])
    assert torch.equal(m.gauss_params["quats"].detach().reshape(-1), flat[6 * n:10 * n])
    # adopting a flat buffer: the same predicate
    adopted = QEDSplatterModel(None, **m.layout.views(flat), flat=flat)
    assert adopted.flat_params is flat and adopted.layout == m.layout
    with pytest.raises(ValueError, match="views of it in GROUP_ORDER"):
        QEDSplatterModel(None, **{**m.layout.views(flat), "scales": flat[3 * n:6 * n].clone().view(n, 3)}, flat=flat)
    sep = QEDSplatterModel(None, separate_params=True, **t)
    assert sep.layout is None and sep.group_begin == []
