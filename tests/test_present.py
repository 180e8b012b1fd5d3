"""GPU tests of csrc/present.hip (qed_present_range, qed_present_frame) against the NumPy restatement in
tests/present_ref.py: every output plane and the range, bit for bit.

Shapes: widths below one lane's four pixels, W % 4 in {0, 1, 2, 3}, rows shorter than, equal to and longer than a wave's
256 pixels, several workgroups.  qed_present_range runs at most 256 workgroups of 8192 pixels (1024 lanes x 2 quads) per
pass, so 2049 x 1024 is the one shape whose frame needs a second pass of that grid (2048 x 1024 fills one exactly); 9 x 257
and 33 x 1021 end inside a workgroup's first or second quad.

The round trip through qed_ingest_ground_truth is asserted to the bound "half a unit plus one float32 ulp of the depth"
at a unit s u that is a power of two (s = 2, u = 2^-11).  There the two scales (float32(1 / (s u)) here, float32(s u) in
the ingest kernel) are exact and so is the product back; the one rounding left besides the quantisation is the fmaf's,
half an ulp of depth / (s u) + 0.5, which is at most one ulp of the depth in units of s u.  For a unit that is not a power
of two the two scale roundings and the product's add up to about another ulp and a half: on the NumPy restatement of
both kernels, at s u = 0.001, 25 of 463 604 unsaturated pixels of twenty 33 x 1021 frames exceed that bound, by at most
0.0007 units (at 0.00073: 124 of 450 457, by at most 0.0017 units).  That is a property of the definitions (float32 scales
on both sides), not of the kernel, which is tested to the bit above."""
from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch

import present_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 3), (3, 5), (2, 64), (5, 67), (7, 256), (9, 257), (33, 1021), (2049, 1024)]
ALL = ("rgb", "depth16", "depthmap", "alpha")
DTYPES = {"rgb": torch.uint8, "depth16": torch.uint16, "depthmap": torch.uint8, "alpha": torch.uint8}
NEAR, FAR = 0.5, 20.0
_FRAMES = {}


def frame(cuda, h, w):
    """Seeded inputs of one size (host and device), their range and both references, made once."""
    if (h, w) not in _FRAMES:
        host = R.inputs(h, w)
        dev = tuple(torch.from_numpy(x).to(cuda) for x in host)
        rng = R.present_range(host[1], host[2])
        refs = {"frame": R.present_frame(*host, R.INV_UNIT_TIES, rng[0], rng[1], R.gray_lut()),
                "host": R.present_frame(*host, R.INV_UNIT_TIES, NEAR, FAR, turbo())}
        _FRAMES[(h, w)] = (host, dev, rng, refs)
    return _FRAMES[(h, w)]


def turbo():
    from qed_splatter_amd.render import colormap
    return colormap("turbo")


def shapes_of(h, w):
    return {"rgb": (h, w, 3), "depth16": (h, w), "depthmap": (h, w, 3), "alpha": (h, w)}


def run(dev, lut, inv_unit, *, per_frame, planes=ALL, offset=False, near=0.0, far=0.0):
    """({plane: numpy}, range numpy | None) through the two entry points; ``offset``: every output starts one element
    behind a fresh allocation."""
    from qed_splatter_amd import _lib as L
    lib = L.load()
    rgb, depth, alpha = dev
    h, w = depth.shape
    outs = {}
    for p in planes:
        shape = shapes_of(h, w)[p]
        n = int(np.prod(shape))
        if offset:
            buf = torch.empty(n + 1, dtype=DTYPES[p], device=rgb.device)
            outs[p] = buf[1:].view(shape)
            assert outs[p].data_ptr() % 4 != 0
        else:
            outs[p] = torch.empty(shape, dtype=DTYPES[p], device=rgb.device)
    lut_t = torch.from_numpy(np.ascontiguousarray(lut)).to(rgb.device)
    st = L.current_stream()
    rng = None
    if per_frame:
        rng = torch.full((2,), 123.0, dtype=torch.float32, device=rgb.device)       # (the call zeroes it itself)
        L.check(lib.qed_present_range(h, w, L.ptr(depth), L.ptr(alpha), L.ptr(rng), st), "qed_present_range")
    L.check(lib.qed_present_frame(h, w, L.ptr(rgb), L.ptr(depth), L.ptr(alpha), float(np.float32(inv_unit)), L.ptr(rng),
                                  near, far, L.ptr(lut_t), L.ptr(outs.get("rgb")), L.ptr(outs.get("depth16")),
                                  L.ptr(outs.get("depthmap")), L.ptr(outs.get("alpha")), st), "qed_present_frame")
    return {p: t.cpu().numpy() for p, t in outs.items()}, (rng.cpu().numpy() if rng is not None else None)


def same(got, want, planes=ALL, tag=""):
    for p in planes:
        assert got[p].shape == want[p].shape and got[p].dtype == want[p].dtype, (tag, p)
        bad = got[p] != want[p]
        assert not bad.any(), f"{tag} {p}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("h,w", SHAPES)
def test_every_plane_bit_for_bit(cuda, h, w):
    host, dev, rng, refs = frame(cuda, h, w)
    got, got_rng = run(dev, R.gray_lut(), R.INV_UNIT_TIES, per_frame=True)
    assert got_rng.tobytes() == rng.tobytes(), (got_rng, rng)
    same(got, refs["frame"], tag=f"{h}x{w} per-frame range")
    got, _ = run(dev, turbo(), R.INV_UNIT_TIES, per_frame=False, near=NEAR, far=FAR)
    same(got, refs["host"], tag=f"{h}x{w} near/far")
    if h * w >= 64:          # the planted specials are there and do what the header says
        d16 = refs["frame"]["depth16"]
        assert (d16 == 0).any() and (d16 == 65535).any() and (refs["frame"]["depthmap"] == 255).all(axis=-1).any()


@pytest.mark.parametrize("h,w", [(5, 67), (9, 257)])
def test_outputs_that_are_not_dword_aligned(cuda, h, w):
    host, dev, rng, refs = frame(cuda, h, w)
    got, got_rng = run(dev, R.gray_lut(), R.INV_UNIT_TIES, per_frame=True, offset=True)
    assert got_rng.tobytes() == rng.tobytes()
    same(got, refs["frame"], tag=f"{h}x{w} offset outputs")
    # and inputs that are float-aligned only
    moved = []
    for t in dev:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        buf[1:] = t.reshape(-1)
        moved.append(buf[1:].view(t.shape))
        assert moved[-1].data_ptr() % 16 != 0
    got, got_rng = run(tuple(moved), R.gray_lut(), R.INV_UNIT_TIES, per_frame=True)
    assert got_rng.tobytes() == rng.tobytes()
    same(got, refs["frame"], tag=f"{h}x{w} offset inputs")


def test_any_subset_of_outputs(cuda):
    h, w = 5, 67
    host, dev, rng, refs = frame(cuda, h, w)
    for k in range(1, 4):
        for planes in itertools.combinations(ALL, k):
            got, _ = run(dev, R.gray_lut(), R.INV_UNIT_TIES, per_frame=True, planes=planes)
            assert sorted(got) == sorted(planes)
            same(got, refs["frame"], planes, tag=f"subset {planes}")
            got, _ = run(dev, R.gray_lut(), R.INV_UNIT_TIES, per_frame=True, planes=planes, offset=True)
            same(got, refs["frame"], planes, tag=f"subset {planes}, per-pixel path")


def test_a_frame_without_a_valid_pixel(cuda):
    h, w = 9, 257
    rgb, depth, alpha = (x.copy() for x in R.inputs(h, w, seed=1))
    alpha[...] = np.where(np.isnan(alpha), alpha, -np.abs(alpha))          # no alpha > 0 (NaN stays)
    dev = tuple(torch.from_numpy(x).to(cuda) for x in (rgb, depth, alpha))
    got, got_rng = run(dev, turbo(), R.INV_UNIT_TIES, per_frame=True)
    assert got_rng.tobytes() == np.zeros(2, np.float32).tobytes()
    assert (got["depthmap"] == 255).all() and (got["depth16"] == 0).all()
    same(got, R.present_frame(rgb, depth, alpha, R.INV_UNIT_TIES, 0.0, 0.0, turbo()), tag="no valid pixel")
    # all depths invalid instead
    rgb, depth, alpha = (x.copy() for x in R.inputs(h, w, seed=2))
    depth[...] = np.where(np.arange(h * w).reshape(h, w) % 3 == 0, np.float32(0), -np.abs(depth))
    depth[1, 1], depth[2, 2] = np.nan, np.inf
    dev = tuple(torch.from_numpy(x).to(cuda) for x in (rgb, depth, alpha))
    got, got_rng = run(dev, turbo(), R.INV_UNIT_TIES, per_frame=True)
    assert got_rng.tobytes() == np.zeros(2, np.float32).tobytes()
    assert (got["depthmap"] == 255).all() and (got["depth16"] == 0).all()


def test_a_frame_of_constant_depth(cuda):
    h, w = 7, 256
    rgb, depth, alpha = (x.copy() for x in R.inputs(h, w, seed=3))
    depth[...] = np.float32(2.5)
    dev = tuple(torch.from_numpy(x).to(cuda) for x in (rgb, depth, alpha))
    got, got_rng = run(dev, turbo(), R.INV_UNIT_TIES, per_frame=True)
    assert got_rng.tobytes() == np.array([2.5, 2.5], np.float32).tobytes()
    want = R.present_frame(rgb, depth, alpha, R.INV_UNIT_TIES, 2.5, 2.5, turbo())
    same(got, want, tag="constant depth")
    # hi == lo: every valid pixel takes entry 0 of the table over white
    opaque = R.valid(depth, alpha) & (alpha >= 1)
    assert opaque.any() and (got["depthmap"][opaque] == turbo()[0]).all()
    assert (got["depth16"][R.valid(depth, alpha)] == 2560).all()


def test_another_unit_and_table(cuda):
    """A unit that is no power of two (millimetres times a dataparser scale of 0.73) and a random table."""
    h, w = 33, 1021
    unit = 0.73 * 0.001
    inv = float(np.float32(1.0 / unit))
    host = R.inputs(h, w, seed=4, inv_unit=inv)
    dev = tuple(torch.from_numpy(x).to(cuda) for x in host)
    lut = np.random.default_rng(5).integers(0, 256, size=(256, 3), dtype=np.uint8)
    rng = R.present_range(host[1], host[2])
    got, got_rng = run(dev, lut, inv, per_frame=True)
    assert got_rng.tobytes() == rng.tobytes()
    same(got, R.present_frame(*host, inv, rng[0], rng[1], lut), tag="unit 0.73 mm")


def test_wrapper_takes_get_outputs_dict(cuda):
    from qed_splatter_amd.render import present_frame
    h, w = 9, 257
    host, dev, rng, refs = frame(cuda, h, w)
    outputs = {"rgb": dev[0], "depth": dev[1][..., None], "accumulation": dev[2][..., None], "background": None}
    got = present_frame(outputs, depth_unit=1.0 / R.INV_UNIT_TIES, lut="gray")
    assert sorted(got) == sorted(ALL) and got["depth16"].dtype == torch.uint16 and got["rgb"].is_cuda
    same({p: t.cpu().numpy() for p, t in got.items()}, refs["frame"], tag="wrapper")
    got = present_frame(outputs, depth_unit=1.0 / R.INV_UNIT_TIES, near=NEAR, far=FAR, planes=("depthmap", "rgb"))
    assert sorted(got) == ["depthmap", "rgb"]
    same({p: t.cpu().numpy() for p, t in got.items()}, refs["host"], ("depthmap", "rgb"), tag="wrapper near/far")
    lut = np.random.default_rng(6).integers(0, 256, size=(256, 3), dtype=np.uint8)
    got = present_frame(outputs, depth_unit=1.0 / R.INV_UNIT_TIES, lut=lut, planes=("depthmap",))
    same({"depthmap": got["depthmap"].cpu().numpy()},
         R.present_frame(*host, R.INV_UNIT_TIES, rng[0], rng[1], lut), ("depthmap",), tag="wrapper own table")
    outputs["depth"] = None                                     # no depth: both depth planes are left out
    got = present_frame(outputs, depth_unit=1.0 / R.INV_UNIT_TIES)
    assert sorted(got) == ["alpha", "rgb"]
    same({p: t.cpu().numpy() for p, t in got.items()}, refs["frame"], ("alpha", "rgb"), tag="wrapper without depth")


def test_round_trip_through_the_ingest_kernel(cuda):
    """out_depth16 at unit s u, read back as a dataset's depth by qed_ingest_ground_truth(depth_scale = s u, d = 1)."""
    from qed_splatter_amd.datamanager import ingest_ground_truth
    h, w = 33, 1021
    s, u = 2.0, 2.0 ** -11
    unit = s * u
    host, dev, rng, refs = frame(cuda, h, w)
    assert R.INV_UNIT_TIES == 1.0 / unit
    from qed_splatter_amd import _lib as L
    d16 = torch.empty(h, w, dtype=torch.uint16, device=cuda)
    L.check(L.load().qed_present_frame(h, w, 0, L.ptr(dev[1]), L.ptr(dev[2]), 1.0 / unit, 0, 0.0, 0.0, 0, 0, L.ptr(d16), 0, 0,
                                       L.current_stream()), "qed_present_frame")
    image = torch.zeros(h, w, 3, dtype=torch.uint8, device=cuda)
    _, back, _ = ingest_ground_truth(image, d16, None, torch.zeros(3, device=cuda), 1, unit)
    back = back[..., 0].cpu().numpy().astype(np.float64)
    depth, alpha = host[1], host[2]
    v = R.valid(depth, alpha)
    assert (back[~v] == 0).all()
    live = v & (d16.cpu().numpy() < 65535)
    err = np.abs(back[live] - depth[live].astype(np.float64))
    bound = 0.5 * unit + np.spacing(depth[live]).astype(np.float64)
    print(f"[present] round trip: {int(live.sum())} pixels, largest error {err.max() / unit:.6f} units, largest excess "
          f"over the bound {((err - bound) / unit).max():.3e} units")
    assert (err <= bound).all()
    assert live.sum() > 0.5 * v.sum() and (~v).sum() > 0
