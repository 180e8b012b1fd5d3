#!/usr/bin/env python3
"""Time per view of the semantic kernels (csrc/semantic.hip) at K = 4, 16, 32 against the passes that exist over the same
tile lists: qed_composite_fwd and qed_contribution (the same walk), ceil(K / 3) passes of qed_composite_fwd over colour slots
(the only route to the same forward image today, as normals.py takes for one triple) and as many passes of
qed_composite_bwd under a colour gradient (what torch autograd through those passes would launch for the table's gradient);
the label kernels against their torch statements; one whole fit step.  HIP events around each call, median / min.

    python scripts/bench_semantic.py [iters] [gaussians width height] [bwd]   (default: config B, 500 000 at 1920x1080)

``bwd`` as the last argument: only qed_features_bwd (for a development build selected with QED_SPLAT_LIB).  Also counted, in
torch float64 on the device, the (tile, Gaussian) pairs with a contributing pixel: the backward's float adds per channel; and
timed, one ``rasterization(colors=table[:, :3], sh_degree=None)`` call with its autograd backward to the colours: what a user
of the public interface pays per colour triple today (projection and binning included).
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from qed_splatter_amd import _lib as L  # noqa: E402
from qed_splatter_amd import semantic as S  # noqa: E402
from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig, get_viewmat  # noqa: E402
from qed_splatter_amd.prune import ContributionScores  # noqa: E402
from qed_splatter_amd.rasterization import rasterization  # noqa: E402
from qed_splatter_amd.scene import synthetic_scene  # noqa: E402

bwd_only = sys.argv[-1] == "bwd"
if bwd_only:
    sys.argv.pop()
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n, w, h = (int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (500_000, 1920, 1080)
dev = torch.device("cuda:0")
lib = L.load()
sc = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in synthetic_scene(n, w, h, seed=1235).items()}
with torch.no_grad():
    _, _, info = rasterization(
        means=sc["means"], quats=torch.nn.functional.normalize(sc["quats"], dim=-1), scales=sc["scales"].exp(),
        opacities=torch.sigmoid(sc["opacities"]).squeeze(-1),
        colors=torch.cat([sc["features_dc"][:, None, :], sc["features_rest"]], dim=1), viewmats=get_viewmat(sc["camera_to_worlds"]),
        Ks=sc["Ks"], width=w, height=h, render_mode="RGB", sh_degree=3, _keep_records=True)
splats, ids, offsets = info["_splats"], info["flatten_ids"], info["_isect_offsets_full"]
tw, th = info["tile_width"], info["tile_height"]
st = L.current_stream()
render = torch.empty(1, h, w, 3, device=dev)
alpha = torch.empty(1, h, w, 1, device=dev)
t_final = torch.empty(1, h, w, device=dev)
last_ids = torch.empty(1, h, w, dtype=torch.int32, device=dev)
tile_cost = torch.empty(tw * th, 4, dtype=torch.int32, device=dev)
order_ws = torch.empty(tw * th + 1, dtype=torch.int32, device=dev)
v_render = torch.ones(1, h, w, 3, device=dev)
v_alpha = torch.zeros(1, h, w, 1, device=dev)
vsplat = torch.zeros(n, L.VSPLAT_FLOATS, device=dev)
scores = ContributionScores(n, dev)


def composite_fwd():
    L.check(lib.qed_composite_fwd(1, n, L.ptr(splats), L.ptr(ids), L.ptr(offsets), w, h, tw, th, 3, None, L.ptr(render),
                                  L.ptr(alpha), L.ptr(t_final), L.ptr(last_ids), L.ptr(tile_cost), None, None, 0, st), "fwd")


def composite_bwd():
    L.check(lib.qed_composite_bwd(1, n, L.ptr(splats), L.ptr(ids), L.ptr(offsets), w, h, tw, th, 3, None, L.ptr(alpha),
                                  L.ptr(t_final), L.ptr(last_ids), L.ptr(v_render), L.ptr(v_alpha), L.ptr(vsplat),
                                  L.ptr(tile_cost), L.ptr(order_ws), None, 0, st), "bwd")


def timed(fn, before=None, reps=None):
    ms = []
    for it in range((reps or iters) + 3):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= 3:
            ms.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(ms), 1), "min_us": round(min(ms), 1)}


result = {"gaussians": n, "width": w, "height": h, "iters": iters, "library": os.environ.get("QED_SPLAT_LIB", "product")}
if bwd_only:
    gen = torch.Generator(device="cpu").manual_seed(0)
    for K in (4, 8, 16, 32):
        v_out = torch.randn(1, h, w, K, generator=gen).to(dev)
        grad = torch.zeros(n, K, device=dev)
        result[f"K={K}"] = {"features_bwd": timed(lambda: S.composite_features_bwd(info, 1, n, v_out, grad, launch_flags=0),
                                                  before=lambda: grad.zero_())}
    print(json.dumps(result))
    sys.exit(0)
result["composite_fwd"] = timed(composite_fwd)
result["contribution"] = timed(lambda: scores.add_view(info, 1, n, w, h, launch_flags=0))
result["composite_bwd_colour_gradient"] = timed(composite_bwd, before=lambda: vsplat.zero_())
runs = torch.diff(offsets[: tw * th + 1].to(torch.int64))
result["list_length"] = int(runs.sum())
result["batches_of_64"] = int(((runs + 63) // 64).sum())


def contributing_pairs():
    """(tile, Gaussian) pairs in which some pixel applies the Gaussian, by the oracle's rule in float64 on the records."""
    rec = splats.reshape(n, -1).double()
    xy, con, op = rec[:, 0:2], rec[:, 2:5], rec[:, 5]
    offs = offsets.reshape(-1).to(torch.int64).tolist()[: tw * th] + [int(ids.numel())]
    ys, xs = torch.meshgrid(torch.arange(16, device=dev), torch.arange(16, device=dev), indexing="ij")
    pairs = 0
    for t in range(tw * th):
        s0, e0 = offs[t], offs[t + 1]
        if e0 <= s0:
            continue
        py, px = ((t // tw) * 16 + ys).reshape(-1), ((t % tw) * 16 + xs).reshape(-1)
        ins = (py < h) & (px < w)
        py, px = py[ins], px[ins]
        g = ids[s0:e0].long()
        dx = xy[g, 0][None, :] - (px.double()[:, None] + 0.5)
        dy = xy[g, 1][None, :] - (py.double()[:, None] + 0.5)
        sigma = 0.5 * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) + con[g, 1] * dx * dy
        a = torch.clamp(op[g][None, :] * torch.exp(-sigma), max=0.999)
        a = torch.where((sigma >= 0) & (a >= 1.0 / 255.0), a, torch.zeros_like(a))
        t_after = torch.cumprod(1.0 - a, dim=1)
        pairs += int(((a > 0) & (t_after > 1e-4)).any(dim=0).sum())
    return pairs


try:
    result["contributing_tile_gaussian_pairs"] = contributing_pairs()
except Exception as exc:                                      # (a measurement aid: its failure must not lose the timings)
    result["contributing_tile_gaussian_pairs"] = f"failed: {exc!r}"


col = torch.randn(n, 3, device=dev).requires_grad_(True)


def autograd_triple():
    col.grad = None
    render, _, _ = rasterization(
        means=sc["means"], quats=torch.nn.functional.normalize(sc["quats"], dim=-1), scales=sc["scales"].exp(),
        opacities=torch.sigmoid(sc["opacities"]).squeeze(-1), colors=col, viewmats=get_viewmat(sc["camera_to_worlds"]),
        Ks=sc["Ks"], width=w, height=h, render_mode="RGB", sh_degree=None)
    render.backward(v_render)


try:
    result["rasterization_autograd_per_colour_triple"] = timed(autograd_triple, reps=5)
except Exception as exc:
    result["rasterization_autograd_per_colour_triple"] = f"failed: {exc!r}"
gen = torch.Generator(device="cpu").manual_seed(0)
for K in (4, 16, 32):
    table = torch.randn(n, K, generator=gen).to(dev)
    v_out = torch.randn(1, h, w, K, generator=gen).to(dev)
    grad = torch.zeros(n, K, device=dev)
    passes = (K + 2) // 3
    r = {"features_fwd": timed(lambda: S.composite_features(info, 1, n, table, launch_flags=0)),
         "features_bwd": timed(lambda: S.composite_features_bwd(info, 1, n, v_out, grad, launch_flags=0),
                               before=lambda: grad.zero_()),
         "colour_slot_passes": passes,
         "composite_fwd_passes": timed(lambda: [composite_fwd() for _ in range(passes)]),
         "composite_bwd_passes": timed(lambda: [composite_bwd() for _ in range(passes)], before=lambda: vsplat.zero_()),
         # one float add per (tile, contributing Gaussian, channel): bounded by the list length
         "atomic_adds_upper_bound": result["list_length"] * K}
    # the label kernels against their torch statements
    logits = S.composite_features(info, 1, n, table, launch_flags=0)[0]
    labels = torch.randint(0, K, (h, w), generator=gen).to(torch.uint8)
    labels[torch.rand(h, w, generator=gen) < 0.2] = 255
    labels = labels.to(dev)
    target = labels.long()
    acc = torch.rand(h, w, generator=gen).to(dev)
    conf = torch.zeros(K, K + 1, dtype=torch.int64, device=dev)
    r["label_loss"] = timed(lambda: S.label_loss(logits, labels))
    x = logits.reshape(-1, K)

    def torch_loss():
        xx = x.detach().requires_grad_(True)
        torch.nn.functional.cross_entropy(xx, target.reshape(-1), ignore_index=255).backward()

    r["torch_cross_entropy_fwd_bwd"] = timed(torch_loss)
    r["label_confusion"] = timed(lambda: S.label_confusion(logits, labels, conf, 255, acc, 0.5))

    def torch_confusion():
        ok = target.reshape(-1) != 255
        pred = torch.where(acc.reshape(-1) >= 0.5, x.argmax(1), K)
        torch.bincount(target.reshape(-1)[ok] * (K + 1) + pred[ok], minlength=K * (K + 1))

    r["torch_confusion"] = timed(torch_confusion)
    result[f"K={K}"] = r

# a whole fit step through the public interface (render + forward + loss + backward + Adam), K = 16
cfg = QEDSplatterModelConfig.synthetic(sh_degree_interval=1)
model = QEDSplatterModel(cfg, **{k: sc[k] for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest")})
model.step = 10000
model.eval()
Kc = sc["Ks"][0]
cam = PinholeCameras(sc["camera_to_worlds"][:1], float(Kc[0, 0]), float(Kc[1, 1]), float(Kc[0, 2]), float(Kc[1, 2]), w, h)
field = S.SemanticField(n, 16, dev)
labels16 = torch.randint(0, 16, (h, w), generator=gen).to(torch.uint8).to(dev)
S.fit(model, [cam], [labels16], field, S.FitConfig(steps=3))
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
S.fit(model, [cam], [labels16], field, S.FitConfig(steps=10))
b.record()
torch.cuda.synchronize()
result["fit_step_K16_ms"] = round(a.elapsed_time(b) / 10, 3)
with torch.no_grad():
    a.record()
    for _ in range(10):
        model.get_outputs(cam)
    b.record()
    torch.cuda.synchronize()
result["evaluation_render_ms"] = round(a.elapsed_time(b) / 10, 3)
print(json.dumps(result))
