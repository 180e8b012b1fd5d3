"""GPU tests of the one-launch ground truth (csrc/ingest.hip, datamanager.ingest_ground_truth, the GpuBatch branch of
QEDSplatterModel._ground_truth) against the float64 restatement in tests/ingest_ref.py.

Bounds, in u = 2^-24, counted from the roundings each path performs (not measured):
  uint8 colour, no alpha   2u absolute      the rounded scale 1 / (255 d^2) and one product, on values <= 1
  uint8 colour with alpha  8u absolute      four such means, then a x rgb + (1 - a) x background: four more roundings
  uint16 depth             4u |value|       the scale as float32, one product
  float32 image / depth    (d^2 + 2) u max|x| over the block      d^2 - 1 additions of values <= max|x|, one product
  mask                     exact            a count times a power of two
The eager route the model comparisons run against is a float32 route too: per pixel k x fl(1/255) (or uint16 x scale),
then a convolution with the exact weight 1 / d^2, i.e. d^2 - 1 additions: (d^2 + 2) u max|x| from the exact value, plus
the composite's roundings (the 8u above) with alpha."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from ingest_ref import DEPTH_SCALE, FACTORS, SHAPES, U, box, inputs, reference

pytestmark = pytest.mark.gpu

CASES = [(h, w, d) for (h, w) in SHAPES for d in FACTORS if h // d > 0 and w // d > 0]
IMAGE_KINDS = ("u8_rgb", "u8_rgba", "f32_rgb")
DEPTH_KINDS = ("u16_depth", "f32_depth")
_FRAMES = {}


def frame(cuda, h, w):
    """The seeded inputs of one size, NumPy and device copies, made once."""
    if (h, w) not in _FRAMES:
        host = inputs(h, w)
        dev = {k: torch.from_numpy(v).to(cuda) for k, v in host.items()}
        _FRAMES[(h, w)] = (host, dev)
    return _FRAMES[(h, w)]


def check(name, got, want, bound):
    err = np.abs(got.double().cpu().numpy().reshape(want.shape) - want)
    worst = float((err - bound).max())
    print(f"[ingest] {name}: max error {err.max() / U:.3f} u, largest excess over its bound {worst / U:.3f} u")
    assert worst <= 0.0, f"{name}: error exceeds its bound by {worst / U:.3f} u"


def bounds(host, image_kind, depth_kind, d, ref_depth):
    if image_kind == "u8_rgb":
        b_rgb = 2 * U
    elif image_kind == "u8_rgba":
        b_rgb = 8 * U
    else:
        b_rgb = (d * d + 2) * U * box(np.abs(host[image_kind]).astype(np.float64), d, np.max)
    if depth_kind == "u16_depth":
        b_depth = 4 * U * np.abs(ref_depth)
    else:
        b_depth = (d * d + 2) * U * box(np.abs(host[depth_kind]).astype(np.float64), d, np.max)
    return b_rgb, b_depth


def run(dev, image_kind, depth_kind, with_mask, d):
    from qed_splatter_amd.datamanager import ingest_ground_truth
    return ingest_ground_truth(dev[image_kind], dev[depth_kind], dev["mask"] if with_mask else None, dev["background"], d,
                               DEPTH_SCALE)


@pytest.mark.parametrize("h,w,d", CASES)
def test_against_float64(cuda, lib, h, w, d):
    host, dev = frame(cuda, h, w)
    for image_kind in IMAGE_KINDS:
        for depth_kind in DEPTH_KINDS:
            for with_mask in (False, True):
                rgb, depth, mask = run(dev, image_kind, depth_kind, with_mask, d)
                assert rgb.shape == (h // d, w // d, 3) and depth.shape == (h // d, w // d, 1)
                r_rgb, r_depth, r_mask = reference(host[image_kind], host[depth_kind], DEPTH_SCALE,
                                                   host["mask"] if with_mask else None, host["background"], d)
                b_rgb, b_depth = bounds(host, image_kind, depth_kind, d, r_depth)
                tag = f"{h}x{w} d={d} {image_kind} {depth_kind} mask={with_mask}"
                check(tag + " rgb", rgb, r_rgb, b_rgb)
                check(tag + " depth", depth, r_depth, b_depth)
                if with_mask:
                    assert mask.shape == (h // d, w // d, 1)
                    assert np.array_equal(mask.double().cpu().numpy()[..., 0], r_mask), tag + " mask"
                else:
                    assert mask is None


@pytest.mark.parametrize("d", [3, 5, 8])
def test_other_factors_take_the_general_kernel(cuda, lib, d):
    h, w = 23, 37
    host, dev = frame(cuda, h, w)
    for image_kind in IMAGE_KINDS:
        for depth_kind in DEPTH_KINDS:
            rgb, depth, mask = run(dev, image_kind, depth_kind, True, d)
            r_rgb, r_depth, r_mask = reference(host[image_kind], host[depth_kind], DEPTH_SCALE, host["mask"],
                                               host["background"], d)
            b_rgb, b_depth = bounds(host, image_kind, depth_kind, d, r_depth)
            check(f"d={d} {image_kind} rgb", rgb, r_rgb, b_rgb)
            check(f"d={d} {depth_kind} depth", depth, r_depth, b_depth)
            # (1 / d^2 is a power of two only for d = 8; otherwise the rounded scale and one product: 2u on values <= 1)
            check(f"d={d} mask", mask, r_mask, 0.0 if d == 8 else 2 * U)


@pytest.mark.parametrize("d", [1, 2])
def test_buffers_that_are_not_dword_aligned(cuda, lib, d):
    """Views that start at an odd byte (uint8 image, mask) or an odd 16-bit element (depth): same values."""
    h, w = 23, 37
    host, dev = frame(cuda, h, w)

    def shifted(t):
        flat = t.reshape(-1)
        buf = torch.empty(flat.numel() + 1, dtype=t.dtype, device=t.device)
        buf[1:] = flat
        out = buf[1:].view(t.shape)
        assert out.is_contiguous() and out.data_ptr() % 4 != 0
        return out

    moved = dict(dev)
    for k in ("u8_rgb", "u16_depth", "mask"):
        moved[k] = shifted(dev[k])
    for a, b in zip(run(dev, "u8_rgb", "u16_depth", True, d), run(moved, "u8_rgb", "u16_depth", True, d)):
        assert torch.equal(a, b)


# ---- against this package's eager route, through the model -----------------------------------------------------------
def make_model(cuda, h, w, **cfg_kw):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    from qed_splatter_amd.scene import synthetic_scene
    sc = synthetic_scene(300, w, h, seed=5)
    cfg = QEDSplatterModelConfig(background_color="random", **cfg_kw)
    model = QEDSplatterModel(cfg, **{k: sc[k].to(cuda) for k in
                                     ("means", "scales", "quats", "opacities", "features_dc", "features_rest")})
    K = sc["Ks"][0]

    def camera():
        return PinholeCameras(sc["camera_to_worlds"][:1].to(cuda), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                              float(K[1, 2]), w, h, metadata={"cam_idx": 0})

    model.train()
    return model, camera


def batches(dev, image_kind, depth_kind, with_mask):
    """(GpuBatch, the equivalent plain dict with float32 depth in metres)."""
    from qed_splatter_amd.datamanager import GpuBatch
    gb = GpuBatch(image=dev[image_kind], depth_image=dev[depth_kind][..., None], image_idx=0,
                  depth_scale=DEPTH_SCALE if depth_kind == "u16_depth" else 1.0)
    depth_f32 = dev[depth_kind][..., None].float() * DEPTH_SCALE if depth_kind == "u16_depth" else dev[depth_kind][..., None]
    plain = {"image": dev[image_kind], "depth_image": depth_f32, "image_idx": 0}
    if with_mask:
        gb["mask"] = plain["mask"] = dev["mask"][..., None]
    return gb, plain


@pytest.mark.parametrize("h,w", SHAPES)
def test_full_resolution_is_bit_identical_to_the_eager_route(cuda, lib, h, w):
    """d = 1: uint8 RGB, float32 depth and the bool mask come out exactly as _ground_truth makes them from a plain dict
    (uint8 -> float is one multiplication by float32(1 / 255) on both routes)."""
    host, dev = frame(cuda, h, w)
    model, _ = make_model(cuda, h, w, num_downscales=0)
    gb, plain = batches(dev, "u8_rgb", "f32_depth", True)
    bg = dev["background"]
    fused, eager = model._ground_truth(gb, bg, h, w), model._ground_truth(plain, bg, h, w)
    for name, a, b in zip(("rgb", "depth", "mask"), fused, eager):
        assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, name
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} values differ"
    # (and 16-bit depth: the float32 view the batch hands every dict consumer is what the kernel computes)
    gb16, _ = batches(dev, "u8_rgb", "u16_depth", False)
    assert torch.equal(model._ground_truth(gb16, bg, h, w)[1], gb16["depth_image"])


@pytest.mark.parametrize("image_kind,depth_kind", [("u8_rgb", "f32_depth"), ("u8_rgba", "u16_depth"), ("f32_rgb", "u16_depth")])
def test_through_the_model_at_every_downscale_factor(cuda, lib, image_kind, depth_kind):
    h, w = 23, 37
    host, dev = frame(cuda, h, w)
    model, camera = make_model(cuda, h, w, num_downscales=2, resolution_schedule=3000)
    gb, plain = batches(dev, image_kind, depth_kind, True)
    bg = dev["background"]
    for step, d in ((0, 4), (3000, 2), (6000, 1)):
        model.step = step
        assert model._get_downscale_factor() == d
        # the size the step renders at (a fresh camera per factor: rescaling a camera whose size the factor does not
        # divide down and back up again does not restore it)
        cam = camera()
        _, _, _, W, H = model._camera_inputs(cam, cam.camera_to_worlds)
        fused, eager = model._ground_truth(gb, bg, H, W), model._ground_truth(plain, bg, H, W)
        r_rgb, r_depth, r_mask = reference(host[image_kind], host[depth_kind], DEPTH_SCALE, host["mask"], host["background"], d)
        b_rgb, b_depth = bounds(host, image_kind, depth_kind, d, r_depth)
        assert fused[0].shape == (H, W, 3) and fused[1].numel() == H * W and fused[2].numel() == H * W
        check(f"model d={d} {image_kind} rgb", fused[0], r_rgb, b_rgb)
        check(f"model d={d} {depth_kind} depth", fused[1], r_depth, b_depth)
        assert np.array_equal(fused[2].double().cpu().numpy()[..., 0], r_mask)
        # the eager float32 route's own distance from the exact value (module docstring), added to the kernel's
        e_rgb = (d * d + 2) * U + (8 * U if image_kind == "u8_rgba" else 0.0)          # (every colour value is <= 1)
        e_depth = (d * d + 2) * U * box(np.abs(reference(host[image_kind], host[depth_kind], DEPTH_SCALE, None,
                                                         host["background"], 1)[1]), d, np.max)
        check(f"model d={d} {image_kind} rgb, fused against eager", fused[0], eager[0].double().cpu().numpy(), b_rgb + e_rgb)
        check(f"model d={d} {depth_kind} depth, fused against eager", fused[1], eager[1].double().cpu().numpy().reshape(H, W),
              b_depth + e_depth)
        assert torch.equal(fused[2], eager[2])


def test_size_mismatch_is_refused_before_the_launch(cuda, lib):
    from qed_splatter_amd import _lib as L
    host, dev = frame(cuda, 23, 37)
    model, camera = make_model(cuda, 16, 16, num_downscales=0)
    cam = camera()
    gb, _ = batches(dev, "u8_rgb", "f32_depth", False)
    with pytest.raises(L.QedSplatError, match="the render is 16x16"):
        model._ground_truth(gb, dev["background"], 16, 16)
    with pytest.raises(L.QedSplatError, match="the render is 16x16"):
        model.fused_loss(cam, gb)


def test_metrics_on_a_gpu_batch_equal_the_plain_dict(cuda, lib):
    """get_metrics_dict indexes the batch: with 16-bit depth it is handed the float32 view, and returns what it returns
    for the equivalent plain dict."""
    h, w = 23, 37
    host, dev = frame(cuda, h, w)
    model, camera = make_model(cuda, h, w, num_downscales=0)
    cam = camera()
    gb, plain = batches(dev, "u8_rgb", "u16_depth", False)
    model.eval()
    with torch.no_grad():
        out = model.get_outputs(cam)
        m_gb, m_plain = model.get_metrics_dict(out, gb), model.get_metrics_dict(out, plain)
    assert list(m_gb) == list(m_plain)
    for k in m_gb:
        a, b = m_gb[k], m_plain[k]
        if torch.is_tensor(a):
            assert torch.equal(a, b) or (bool(torch.isnan(a).all()) and bool(torch.isnan(b).all())), k
        else:
            assert a == b, k
    # and the loss route runs on it: fused kernel for the GpuBatch, eager chain for the dict, the same numbers
    model.train()
    bg = dev["background"]
    l_gb, l_plain = model.fused_loss(cam, gb, background=bg), model.fused_loss(cam, plain, background=bg)
    for k in ("main_loss", "depth_loss"):
        assert torch.equal(l_gb[k], l_plain[k]), k
