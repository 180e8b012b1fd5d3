"""The semantic kernels (qed_features_fwd / qed_features_bwd / qed_label_loss / qed_label_confusion / qed_label_present)
through the C ABI and semantic.py's public interface.  The walking kernels run on the crafted tile lists of
tests/composite_cases.py (records and lists from tests/test_composite_edges._setup) against the float64 oracle of
tests/semantic_ref.py on the kernels' own float32 records, for channel counts on both sides of every chunk size; the label
kernels on 17x9 and 64x48 images with the CPU test's crafted label maps; fit / evaluate / render / prune / PLY on a 64x48
synthetic model.  Run with `pytest -m gpu` on an MI355X."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import splat_oracle as O
from tests import adam_ref as A
from tests import composite_cases as K
from tests import semantic_ref as R
from tests.test_train_dataset import dataset  # noqa: F401  (the trainer tests' tiny dataset: a module-scoped fixture)
from tests.test_composite_edges import _setup          # the cases' projection and lists on the device, shared and read-only
from tests.util import PARAM_NAMES, REL_TOL, assert_close, assert_close_elem, scene

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.0
_REF = {}


def _ref(name, k, dev):
    """Once per (case, K): the table, the oracle's image of it on the kernels' float32 records, a random upstream gradient
    that is zero on the unsafe pixels, and the autograd gradient of the table."""
    key = (name, k)
    if key in _REF:
        return _REF[key]
    d = _setup(name, dev)
    c = d.c
    m2, con, _, op, _ = (t.detach() for t in d.ins64)
    F = R.table(c.N, k).float().double().requires_grad_(True)           # (float32 values, as the kernel reads them)
    out, _ = R.forward(c, m2, con, op, F)
    g = torch.Generator().manual_seed(len(name) + 100 * k)
    v = torch.randn(c.C, c.h, c.w, k, generator=g, dtype=torch.float64).float().double() * d.safe[..., None].double()
    grad = torch.autograd.grad((out * v).sum(), F)[0] if c.M else torch.zeros_like(F)
    _REF[key] = r = (d, F.detach(), out.detach(), v, grad)
    return r


def _guarded(n, dev, fill=SENTINEL):
    """n floats of a sentinel for a kernel to fill, and GUARD words behind them that it must leave alone."""
    buf = torch.full((n + GUARD,), fill, dtype=torch.float32, device=dev)
    buf[n:] = torch.arange(1, GUARD + 1, device=dev)
    return buf


def _guard_intact(buf):
    return torch.equal(buf[-GUARD:], torch.arange(1, GUARD + 1, device=buf.device, dtype=buf.dtype))


def _forward(d, F, dev, flags=0, null_list=False):
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import _stream
    c = d.c
    k = F.shape[1]
    n = c.C * c.h * c.w * k
    buf = _guarded(n, dev)
    table = F.to(dev, torch.float32).contiguous()
    L.check(L.load().qed_features_fwd(c.C, c.N, k, L.ptr(d.splats), None if null_list else L.ptr(d.fid), L.ptr(d.offs), c.w,
                                      c.h, c.tile_w, c.tile_h, L.ptr(table), L.ptr(buf), flags, _stream()), "qed_features_fwd")
    torch.cuda.synchronize()
    assert _guard_intact(buf), "qed_features_fwd wrote behind its image"
    return buf[:n].view(c.C, c.h, c.w, k)


def _backward(d, v, k, dev, flags=0, into=None):
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import _stream
    c = d.c
    buf = _guarded(c.N * k, dev, 0.0) if into is None else into
    v32 = v.to(dev, torch.float32).contiguous()
    L.check(L.load().qed_features_bwd(c.C, c.N, k, L.ptr(d.splats), L.ptr(d.fid), L.ptr(d.offs), c.w, c.h, c.tile_w, c.tile_h,
                                      L.ptr(v32), L.ptr(buf), flags, _stream()), "qed_features_bwd")
    torch.cuda.synchronize()
    assert _guard_intact(buf), "qed_features_bwd wrote behind the table's gradient"
    return buf


CASES = pytest.mark.parametrize("name", K.NAMES)
CHANNELS = pytest.mark.parametrize("k", R.CHANNELS)


@CHANNELS
@CASES
def test_forward_against_oracle(cuda, name, k):
    """out against the oracle on the safe pixels at the project's 1e-4; exact zeros in empty tiles; every in-image value
    written, nothing behind the image; the same bits with the culling off."""
    from qed_splatter_amd import _lib as L
    d, F, want, _, _ = _ref(name, k, cuda)
    share = 1.0 - float(d.safe.double().mean())
    assert share <= R.MAX_UNSAFE_SHARE, f"{name}: {share:.4%} of the pixels sit on a threshold in float32"
    got = _forward(d, F, cuda)
    assert bool((got != SENTINEL).all()), "a pixel inside the image was not written"
    out = got.cpu()
    if d.c.M:
        assert_close(out[d.safe], want[d.safe], REL_TOL, f"{name}/K={k}: out")
        assert_close_elem(out[d.safe], want[d.safe], f"{name}/K={k}: out", atol_frac=1e-5)
    e = d.empty_pixel
    assert bool(e.any()) == bool((d.lens == 0).any())
    assert bool((out[e] == 0).all()), "an empty tile's pixels must be exactly zero"
    if name == "empty_all":
        assert bool((out == 0).all())
    assert torch.equal(_forward(d, F, cuda, L.CL_NO_CULL), got), "QED_CL_NO_CULL changed bits of the forward"


@CHANNELS
@CASES
def test_backward_against_autograd(cuda, name, k):
    """Every element of v_features against the oracle's autograd gradient; rows of Gaussians that never contribute stay
    exactly zero; a second call without re-zeroing doubles the result."""
    from qed_splatter_amd import _lib as L
    d, F, _, v, want = _ref(name, k, cuda)
    c = d.c
    buf = _backward(d, v, k, cuda)
    got = buf[:c.N * k].view(c.N, k).cpu()
    if c.M:
        assert float(want.abs().max()) > 0
        assert_close(got, want, REL_TOL, f"{name}/K={k}: v_features")
        assert_close_elem(got, want, f"{name}/K={k}: v_features", atol_frac=1e-5)
    else:
        assert bool((got == 0).all())
    never = (want == 0).all(dim=1)                        # (no weight at any safe pixel: at most exact zeros were added)
    assert bool((got[never] == 0).all())
    once = buf[:c.N * k].clone()
    twice = _backward(d, v, k, cuda, into=buf)[:c.N * k]
    assert_close(twice, 2.0 * once.double(), 2e-6, f"{name}/K={k}: accumulation")
    assert_close(_backward(d, v, k, cuda, L.CL_NO_CULL)[:c.N * k], once, 2e-6, f"{name}/K={k}: culling off")


@pytest.mark.parametrize("name", ("culled_batches_lane0", "far_only", "quadrant_endings", "mixed_forms"))
def test_far_entries_issue_no_add(cuda, name):
    """Gaussians that the lists name only as far entries (no pixel of any listing tile reaches alpha >= 1/255): their rows
    keep the bits they had, a NaN-free sentinel included -- no add was issued for them."""
    d = _setup(name, cuda)
    c = d.c
    cen = K.census(c, d.means2d.cpu(), d.conics.cpu(), d.opac.cpu())
    fid = c.flatten_ids.to(torch.int64)
    touched = torch.zeros(c.N, dtype=torch.bool)
    listed = torch.zeros(c.N, dtype=torch.bool)
    for t in cen:
        if t["length"]:
            g = fid[t["start"]:t["start"] + t["length"]] % c.N
            listed[g] = True
            touched[g[torch.from_numpy(t["touch"].any(1))]] = True
    far_only = listed & ~touched
    assert int(far_only.sum()) >= 19
    k = 5
    buf = _guarded(c.N * k, cuda, 0.0)
    buf[:c.N * k].view(c.N, k)[far_only.to(cuda)] = SENTINEL
    v = torch.ones(c.C, c.h, c.w, k, dtype=torch.float64)
    got = _backward(d, v, k, cuda, into=buf)[:c.N * k].view(c.N, k).cpu()
    assert bool((got[far_only] == SENTINEL).all())
    assert bool((got[listed & ~far_only] >= 0).all())
    if bool(touched.any()):
        assert float(got[touched].max()) > 0


def test_two_cameras_share_the_rows(cuda):
    """Records c N + n of both cameras read and add to row n: the two-camera gradient is the sum of each camera's own."""
    d, F, want_out, v, want = _ref("two_cameras", 5, cuda)
    c = d.c
    assert c.C == 2 and float(want.abs().max()) > 0
    both = _backward(d, v, 5, cuda)[:c.N * 5].cpu()
    parts = []
    for cam in range(2):
        vc = v.clone()
        vc[1 - cam] = 0
        parts.append(_backward(d, vc, 5, cuda)[:c.N * 5].cpu().double())
    assert float(parts[0].abs().max()) > 0 and float(parts[1].abs().max()) > 0
    assert_close(both, parts[0] + parts[1], 2e-6, "two cameras: sum of the cameras' gradients")


def test_without_a_list_the_image_is_zero(cuda):
    d, F, _, v, _ = _ref("empty_all", 3, cuda)
    assert bool((_forward(d, F, cuda, null_list=True) == 0).all())


def test_walk_refusals(cuda):
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.rasterization import _stream
    d = _setup("seams", cuda)
    c = d.c
    t = torch.zeros(c.N * 33, device=cuda)
    out = torch.zeros(c.C * c.h * c.w * 33, device=cuda)
    for k, tw, match in ((33, c.tile_w, "channel count"), (0, c.tile_w, "channel count"), (3, c.tile_w + 1, "tile grid")):
        for fn in ("qed_features_fwd", "qed_features_bwd"):
            a, b = (t, out) if fn == "qed_features_fwd" else (out, t)
            with pytest.raises(L.QedSplatError, match=match):
                L.check(getattr(L.load(), fn)(c.C, c.N, k, L.ptr(d.splats), L.ptr(d.fid), L.ptr(d.offs), c.w, c.h, tw, c.tile_h,
                                              L.ptr(a), L.ptr(b), 0, _stream()), fn)


# ---- the label kernels -----------------------------------------------------------------------------------------------------
SIZES = pytest.mark.parametrize("size", [(9, 17), (48, 64)], ids=["17x9", "64x48"])
CLASSES = pytest.mark.parametrize("k", (1, 2, 19, 32))


@pytest.mark.parametrize("weighted", (False, True), ids=["plain", "weighted"])
@pytest.mark.parametrize("kind", R.LABEL_MAPS)
@CLASSES
@SIZES
def test_label_loss_against_float64(cuda, size, k, kind, weighted):
    from qed_splatter_amd import _lib as L
    from qed_splatter_amd.semantic import label_loss
    h, w = size
    x = R.logits_image(h, w, k)
    lab = R.label_map(kind, h, w, k)
    cw = R.class_weights(k) if weighted else None
    want, want_grad = R.cross_entropy(x, lab, R.IGNORE, cw)
    ws = torch.full((L.LABEL_LOSS_WS_DOUBLES,), float("nan"), dtype=torch.float64, device=cuda)
    runs = []
    for _ in range(2):
        loss, grad = label_loss(x.to(cuda), lab.to(cuda), R.IGNORE, None if cw is None else cw.to(cuda), True, ws)
        runs.append((loss.clone(), grad.clone(), ws[-2:].clone()))
    loss, grad, tail = runs[0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), "two runs differ in some bit"
    n_lab = int(R.labelled(lab, k).sum())
    if n_lab == 0:
        assert float(loss) == 0.0 and bool((grad == 0).all()) and float(tail[1]) == 0.0
        return
    print(f"[label loss] {w}x{h} K={k} {kind}: loss {float(loss):.6f} against {float(want):.6f}")
    assert abs(float(loss) - float(want)) <= REL_TOL * abs(float(want))
    assert_close_elem(grad.reshape(-1, k), want_grad, f"{w}x{h} K={k} {kind}: v_logits")
    assert bool((grad.reshape(-1, k).cpu()[~R.labelled(lab, k)] == 0).all())
    # without v_logits only the value is written, with the same bits
    loss3, none = label_loss(x.to(cuda), lab.to(cuda), R.IGNORE, None if cw is None else cw.to(cuda), False)
    assert none is None and torch.equal(loss3, loss)


@CLASSES
@SIZES
def test_label_confusion_counts_exactly(cuda, size, k):
    """The table equals the reference's integers, with argmax ties (a duplicated column) and the below-min_alpha column;
    calls add up."""
    from qed_splatter_amd.semantic import label_confusion
    h, w = size
    x = R.logits_image(h, w, k)
    if k > 1:
        x[..., k - 1] = x[..., 0]                       # ties between the first and the last class -> the first
    lab = R.label_map("beyond_k", h, w, k)
    g = torch.Generator().manual_seed(k + h)
    acc = torch.rand(h, w, generator=g)
    acc[0, :3] = torch.tensor([0.5, 0.49999997, float("nan")])          # at the bound: a prediction; below; NaN: none
    for a in (None, acc):
        want = R.confusion(x, lab, R.IGNORE, a, 0.5)
        conf = torch.zeros(k, k + 1, dtype=torch.int64, device=cuda)
        label_confusion(x.to(cuda), lab.to(cuda), conf, R.IGNORE, None if a is None else a.to(cuda), 0.5)
        assert torch.equal(conf.cpu(), want)
        if a is None:
            assert int(conf[:, k].sum()) == 0
            if k > 1:
                assert int(conf[:, k - 1].sum()) == 0 and int(conf[:, 0].sum()) > 0, "ties go to the lower index"
        else:
            assert int(conf[:, k].sum()) > 0
        label_confusion(x.to(cuda), lab.to(cuda), conf, R.IGNORE, None if a is None else a.to(cuda), 0.5)
        assert torch.equal(conf.cpu(), 2 * want)


def test_label_present_planes(cuda):
    from qed_splatter_amd.semantic import default_palette, present_labels
    h, w, k = 9, 17, 5
    x = R.logits_image(h, w, k)
    x[..., 3] = x[..., 1]
    g = torch.Generator().manual_seed(3)
    acc = torch.rand(h, w, generator=g)
    pal = default_palette(k)
    label, rgb = present_labels(x.to(cuda), acc.to(cuda), pal, 0.5)
    pred = torch.where(x == x.amax(-1, keepdim=True), torch.arange(k), torch.tensor(k)).amin(-1)
    want = torch.where(acc >= 0.5, pred, torch.tensor(255))
    assert label.dtype == torch.uint8 and torch.equal(label.cpu().long(), want)
    assert torch.equal(rgb.cpu(), pal[torch.where(acc >= 0.5, pred, torch.tensor(k))])
    label2, _ = present_labels(x.to(cuda), None, pal)
    assert torch.equal(label2.cpu().long(), pred)


# ---- the public interface on a model ---------------------------------------------------------------------------------------
W, H = 64, 48


def _scene(backdrop: bool = False, seed: int = 21):
    """A 64x48 synthetic scene of 600 Gaussians seen by two cameras; with ``backdrop`` 48 broad, nearly opaque Gaussians on
    an 8-pixel grid 9 units in front of camera 0, behind everything else, so that every pixel of camera 0 accumulates more
    than 0.5."""
    sc = scene(600, W, H, seed=seed, n_cameras=2)
    sc["scales"] = sc["scales"] + 1.0
    if backdrop:
        Kc, c2w = sc["Ks"][0].double(), sc["camera_to_worlds"][0].double()
        depth = 9.0
        px, py = torch.meshgrid(torch.arange(4.0, W, 8.0), torch.arange(4.0, H, 8.0), indexing="xy")
        px, py = px.reshape(-1).double(), py.reshape(-1).double()
        cam = torch.stack([(px - Kc[0, 2]) / Kc[0, 0] * depth, -(py - Kc[1, 2]) / Kc[1, 1] * depth,
                           torch.full_like(px, -depth)], dim=1)             # OpenGL camera: looks down -z, y up
        world = (c2w[:3, :3] @ cam.T).T + c2w[:3, 3]
        n = world.shape[0]
        extra = {"means": world.float(), "scales": torch.full((n, 3), float(np.log(8.0 * depth / float(Kc[0, 0])))),
                 "quats": torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(n, 1), "opacities": torch.full((n, 1), 4.0),
                 "features_dc": torch.zeros(n, 3), "features_rest": torch.zeros(n, sc["features_rest"].shape[1], 3)}
        for name in PARAM_NAMES:
            sc[name] = torch.cat([sc[name], extra[name].to(sc[name].dtype)])
    return sc


def _model(sc, dev):
    from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig
    m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(sh_degree_interval=1), **{k: sc[k].to(dev) for k in PARAM_NAMES})
    m.step = 100
    m.eval()
    Kc = sc["Ks"][0]
    cams = [PinholeCameras(sc["camera_to_worlds"][k:k + 1].to(dev), float(Kc[0, 0]), float(Kc[1, 1]), float(Kc[0, 2]),
                           float(Kc[1, 2]), W, H) for k in range(sc["camera_to_worlds"].shape[0])]
    return m, cams


def _records(model, cam):
    """The float32 records and lists of one evaluation render, on the CPU in float64, as the oracle takes them."""
    from qed_splatter_amd.semantic import _Frozen
    with torch.no_grad(), _Frozen(model) as fr:
        info, acc, h, w = fr.render(cam)
        rec = {k: info[k].detach().cpu() for k in ("means2d", "conics", "opacities", "flatten_ids", "isect_offsets")}
        fr.release(info)
    assert (h, w) == (H, W) and "_splats" not in model.info
    return rec, acc.cpu()


def _oracle_logits(rec, F):
    out, _, _, margin = O.composite_tiles(rec["means2d"].double(), rec["conics"].double(), F[None], rec["opacities"].double(),
                                          W, H, 16, rec["isect_offsets"], rec["flatten_ids"], return_margin=True)
    return out[0], margin[0]


def test_render_logits_against_oracle(cuda):
    from qed_splatter_amd.semantic import SemanticField, render_logits
    model, cams = _model(_scene(), cuda)
    field = SemanticField(model.num_points, 5, cuda)
    field.logits.copy_(R.table(model.num_points, 5).float())
    logits, acc = render_logits(model, cams[1], field)
    assert tuple(logits.shape) == (H, W, 5) and tuple(acc.shape) == (H, W) and "_splats" not in model.info
    rec, _ = _records(model, cams[1])
    want, margin = _oracle_logits(rec, field.logits.cpu().double())
    safe = margin > R.MARGIN
    assert float(safe.double().mean()) >= 0.99
    assert_close(logits.cpu()[safe], want[safe], REL_TOL, "render_logits")
    with pytest.raises(ValueError, match="the model has"):
        render_logits(model, cams[0], SemanticField(model.num_points + 1, 5, cuda))
    model.train()
    with pytest.raises(NotImplementedError, match="captured step"):
        render_logits(model, cams[0], field, captured_step=object())
    model.eval()


def test_one_fit_step_is_adams_first_step(cuda):
    """fit(steps=1) from a random table: the new table against Adam's first step (tests/adam_ref.py, at its update bound)
    from the oracle's gradient of the cross-entropy on the render's own float32 records.  Pixels whose decisions sit on a
    threshold are unlabelled (255), so both sides see the same pixels."""
    from qed_splatter_amd.semantic import FitConfig, SemanticField, fit
    model, cams = _model(_scene(), cuda)
    k, lr = 3, 0.05
    N = model.num_points
    rec, _ = _records(model, cams[0])
    F0 = R.table(N, k).float()
    F = F0.double().requires_grad_(True)
    logits, margin = _oracle_logits(rec, F)
    lab = R.label_map("mixed", H, W, k)
    lab[~(margin > R.MARGIN)] = R.IGNORE
    _, v = R.cross_entropy(logits.detach(), lab)
    grad, = torch.autograd.grad((logits.reshape(-1, k) * v).sum(), F)
    assert int((grad != 0).any(dim=1).sum()) > 100
    field = SemanticField(N, k, cuda)
    field.logits.copy_(F0)
    hist = fit(model, cams[:1], [lab.to(cuda)], field, FitConfig(steps=1, lr=lr, eps=A.EPS))
    want_loss, _ = R.cross_entropy(logits.detach(), lab)
    assert len(hist) == 1 and abs(hist[0] - float(want_loss)) <= REL_TOL * float(want_loss)
    assert field.step == 1 and not model.training
    ref = A.adam_ref(F0.reshape(-1), grad.reshape(-1), torch.zeros(N * k), torch.zeros(N * k), [0, N * k], [lr], *A.BETAS,
                     A.EPS, 1)
    e = A.step_errors(field.logits.reshape(-1), field.exp_avg.reshape(-1), field.exp_avg_sq.reshape(-1), F0.reshape(-1), ref)
    print(f"[semantic] one fit step: update {e['update']:.2e} (tol {A.TOL_UPDATE:.1e}), exp_avg {e['exp_avg']:.2e}")
    assert e["update"] <= A.TOL_UPDATE
    untouched = (grad == 0).all(dim=1)
    assert bool(untouched.any()) and torch.equal(field.logits.cpu()[untouched], F0[untouched])
    assert_close(field.exp_avg.cpu(), ref[1].reshape(N, k), REL_TOL, "exp_avg")


def test_fit_refusals_come_before_any_launch(cuda):
    from qed_splatter_amd.semantic import FitConfig, SemanticField, fit
    model, cams = _model(_scene(), cuda)
    field = SemanticField(model.num_points, 3, cuda)
    with pytest.raises(ValueError, match="resizing is not offered"):
        fit(model, cams[:1], [torch.zeros(H, W + 1, dtype=torch.uint8)], field, FitConfig(steps=1))
    with pytest.raises(ValueError, match="class weights"):
        fit(model, cams[:1], [torch.zeros(H, W, dtype=torch.uint8)], field, FitConfig(steps=1, class_weight=[1.0, 2.0]))
    assert field.step == 0 and bool((field.logits == 0).all())


def test_fit_on_constant_labels(cuda):
    """Every pixel labelled class 1 (K = 3), 30 steps: every pixel with accumulation >= 0.5 predicts class 1, evaluate reports
    pixel_accuracy == 1.0 and an all-diagonal confusion matrix (the backdrop makes every pixel accumulate more than 0.5)."""
    from qed_splatter_amd.semantic import FitConfig, SemanticField, evaluate, fit, render_logits
    model, cams = _model(_scene(backdrop=True), cuda)
    field = SemanticField(model.num_points, 3, cuda)
    lab = torch.ones(H, W, dtype=torch.uint8, device=cuda)
    hist = fit(model, cams[:1], [lab], field, FitConfig(steps=30))
    assert len(hist) == 30 and hist[-1] < hist[0] and abs(hist[0] - float(np.log(3.0))) < 1e-5
    logits, acc = render_logits(model, cams[0], field)
    assert float(acc.min()) >= 0.5, "the scene was built to cover camera 0"
    assert bool((logits.argmax(-1)[acc >= 0.5] == 1).all())
    res = evaluate(model, cams[:1], [lab], field, min_alpha=0.5)
    assert res["pixel_accuracy"] == 1.0 and res["miou"] == 1.0
    assert res["confusion"] == [[0, 0, 0, 0], [0, H * W, 0, 0], [0, 0, 0, 0]]
    assert res["per_class_iou"] == [None, 1.0, None]


def test_field_file_prune_and_ply_round_trips(cuda, tmp_path):
    from qed_splatter_amd.gaussian_ply import export_gaussian_ply, load_gaussians, read_gaussian_ply
    from qed_splatter_amd.prune import PruneConfig, keep_mask, prune, score_views
    from qed_splatter_amd.semantic import SemanticField, gaussian_labels
    model, cams = _model(_scene(), cuda)
    N = model.num_points
    field = SemanticField(N, 4, cuda, class_names=["terrain", "obstacle", "sky", "person"])
    field.logits.copy_(R.table(N, 4).float())
    field.exp_avg.copy_(R.table(N, 4, seed=1).float())
    field.exp_avg_sq.copy_(R.table(N, 4, seed=2).float() ** 2)
    field.step = 7
    field.save(tmp_path / "field.pt")
    back = SemanticField.load(tmp_path / "field.pt", cuda)
    for a, b in ((back.logits, field.logits), (back.exp_avg, field.exp_avg), (back.exp_avg_sq, field.exp_avg_sq)):
        assert torch.equal(a, b)
    assert back.step == 7 and back.class_names == field.class_names and torch.equal(back.palette, field.palette)
    # the PLY with a label property is read back by the existing importer with the same Gaussians
    labels = gaussian_labels(field)
    plain = export_gaussian_ply(model, tmp_path / "plain.ply")
    res = export_gaussian_ply(model, tmp_path / "labelled.ply", labels=labels)
    assert res == plain and res["written"] > 0
    a, b = load_gaussians(tmp_path / "plain.ply", device=cuda), load_gaussians(tmp_path / "labelled.ply", device=cuda)
    for name in PARAM_NAMES:
        assert torch.equal(a[name], b[name]), name
    ply = read_gaussian_ply(tmp_path / "labelled.ply")
    kept = model.opacities.reshape(-1) >= torch.tensor(-5.5373, dtype=torch.float32)
    assert ply.n == int(kept.sum()) and np.array_equal(ply.column("label"), labels[kept].cpu().numpy())
    assert read_gaussian_ply(tmp_path / "plain.ply").row_bytes + 1 == ply.row_bytes
    # prune(..., field=) keeps the survivors' rows bit for bit
    scores = score_views(model, cams)
    cfg = PruneConfig(score="max", min_score=0.05)
    keep = keep_mask(cfg, scores.max_weight(), scores.sum_weight(), model.scales)
    assert 0 < int(keep.sum()) < N
    info = prune(model, None, scores, cfg, field=field)
    pruned = info["field"]
    assert info["n_after"] == int(keep.sum()) == pruned.n_gaussians == model.num_points
    for a, b in ((pruned.logits, field.logits), (pruned.exp_avg, field.exp_avg), (pruned.exp_avg_sq, field.exp_avg_sq)):
        assert torch.equal(a, b[keep])
    assert pruned.step == 7
    with pytest.raises(ValueError, match="the model has"):
        prune(model, None, score_views(model, cams), cfg, field=field)


def test_render_semantic_planes(cuda, tmp_path):
    """render.py's "semantic" plane on a 33x17 view: both PNGs, the class byte = the argmax of render_logits where the
    accumulation reaches 0.5 and 255 elsewhere, the colours = the palette's; the plane without a field is refused by name."""
    from PIL import Image
    from qed_splatter_amd.model import PinholeCameras
    from qed_splatter_amd.render import render_to_directory
    from qed_splatter_amd.semantic import SemanticField, render_logits
    sc = _scene()
    model, _ = _model(sc, cuda)
    Kc = sc["Ks"][0]
    s = 33.0 / W
    cam = PinholeCameras(sc["camera_to_worlds"][:1].to(cuda), float(Kc[0, 0]) * s, float(Kc[1, 1]) * s, 16.5, 8.5, 33, 17)
    field = SemanticField(model.num_points, 5, cuda)
    field.logits.copy_(R.table(model.num_points, 5).float())
    with pytest.raises(ValueError, match="'semantic' needs a field"):
        render_to_directory(model, [cam], tmp_path / "none", depth_unit=1e-3, planes=("rgb", "semantic"))
    res = render_to_directory(model, [cam], tmp_path / "out", depth_unit=1e-3, planes=("rgb", "semantic"), field=field)
    assert res["frames"] == 1 and "_score_records" not in model.__dict__ and "_splats" not in model.info
    label = np.array(Image.open(tmp_path / "out" / "semantic_label" / "00000.png"))
    rgb = np.array(Image.open(tmp_path / "out" / "semantic" / "00000.png"))
    assert label.shape == (17, 33) and label.dtype == np.uint8 and rgb.shape == (17, 33, 3)
    assert (tmp_path / "out" / "rgb" / "00000.png").exists()
    logits, acc = render_logits(model, cam, field)
    seen = (acc >= 0.5).cpu().numpy()
    assert seen.any() and (~seen).any()
    pred = logits.argmax(-1).cpu().numpy()
    assert np.array_equal(label[seen], pred[seen]) and (label[~seen] == 255).all()
    pal = field.palette.cpu().numpy()
    assert np.array_equal(rgb, pal[np.where(seen, pred, 5)])
    # beside the normal plane (whose pass also reads the render's records), and on a model that renders normals anyway
    for planes, flag in ((("normal", "semantic"), False), (("semantic",), True)):
        model.config.output_normals = flag
        out = tmp_path / ("with_normal" if not flag else "normals_on")
        res = render_to_directory(model, [cam], out, depth_unit=1e-3, planes=planes, field=field)
        assert res["frames"] == 1 and "_splats" not in model.info and model.config.output_normals is flag
        assert np.array_equal(np.array(Image.open(out / "semantic_label" / "00000.png")), label)
        assert np.array_equal(np.array(Image.open(out / "semantic" / "00000.png")), rgb)
        assert (out / "normal" / "00000.png").exists() == ("normal" in planes)
    model.config.output_normals = False


def test_labelled_ply_refusals_leave_no_file(cuda, tmp_path):
    from qed_splatter_amd.gaussian_ply import export_gaussian_ply
    model, _ = _model(_scene(), cuda)
    with pytest.raises(ValueError, match="one class per Gaussian"):
        export_gaussian_ply(model, tmp_path / "a.ply", labels=torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="one class per Gaussian"):
        export_gaussian_ply(model, tmp_path / "a.ply", labels=torch.zeros(model.num_points, dtype=torch.int64))
    assert not (tmp_path / "a.ply").exists()


def test_fit_and_eval_command_line(cuda, dataset, tmp_path, capsys):  # noqa: F811
    """train --save, then `semantic fit` and `semantic eval` on a copy of the trainer tests' dataset whose frames carry
    constant label images: one JSON line each, a field file that loads, and a class count inferred from the labels."""
    import json
    import shutil
    from PIL import Image
    from qed_splatter_amd import semantic as S
    from qed_splatter_amd import train
    src, _ = dataset
    root = tmp_path / "data"
    shutil.copytree(src, root)
    meta = json.loads((root / "transforms.json").read_text())
    (root / "labels").mkdir()
    for i, f in enumerate(meta["frames"]):
        with Image.open(root / f["file_path"]) as im:
            w, h = im.size
        lab = np.full((h, w), 2, dtype=np.uint8)
        lab[:2] = 255
        Image.fromarray(lab).save(root / "labels" / f"{i:03d}.png")
        f["label_path"] = f"labels/{i:03d}.png"
    (root / "transforms.json").write_text(json.dumps(meta))
    common = ["--data", str(root), "--orientation-method", "none", "--center-method", "none", "--auto-scale-poses", "False",
              "--train-split-fraction", "0.8"]
    ckpt, field_path, report = tmp_path / "a.pt", tmp_path / "field.pt", tmp_path / "report.json"
    train.main(common + ["--steps", "5", "--seed", "1", "--save", str(ckpt)])
    capsys.readouterr()
    res = S.main(["fit", *common, "--load", str(ckpt), "--output", str(field_path), "--steps", "12", "--stride", "2"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["n_classes"] == res["n_classes"] == 3 and line["steps"] == 12 and line["last_loss"] < line["first_loss"]
    field = S.SemanticField.load(field_path, cuda)
    assert field.n_classes == 3 and field.step == 12 and field.n_gaussians > 0
    res = S.main(["eval", *common, "--load", str(ckpt), "--field", str(field_path), "--split", "all", "--output-path",
                  str(report)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert json.loads(report.read_text()) == line and line["views"] == len(meta["frames"])
    conf = torch.tensor(line["confusion"])
    assert tuple(conf.shape) == (3, 4) and int(conf[:2].sum()) == 0 and int(conf[2].sum()) > 0
    assert int(conf[2, 2]) > 0 and line["pixel_accuracy"] > 0
