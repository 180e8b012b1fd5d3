#!/usr/bin/env python3
"""Time per view of qed_contribution (csrc/importance.hip) against the two existing passes over the same tile lists:
qed_composite_fwd (the yardstick: the same walk with colours and image writes) and the only other route to the sum of
weights, qed_composite_bwd under a unit colour gradient.  HIP events around each call, median / min over the iterations.

    python scripts/bench_importance.py [iters] [gaussians width height]        (default: config B, 500 000 at 1920x1080)

Also prints the list length, the number of 64-entry batches (an upper bound of the atomic wave instructions per view is
3 per batch: one per quantity) and how many Gaussians the view scores above zero.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from qed_splatter_amd import _lib as L  # noqa: E402
from qed_splatter_amd.model import get_viewmat  # noqa: E402
from qed_splatter_amd.prune import ContributionScores  # noqa: E402
from qed_splatter_amd.rasterization import rasterization  # noqa: E402
from qed_splatter_amd.scene import synthetic_scene  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 30
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


def forward():
    L.check(lib.qed_composite_fwd(1, n, L.ptr(splats), L.ptr(ids), L.ptr(offsets), w, h, tw, th, 3, None, L.ptr(render),
                                  L.ptr(alpha), L.ptr(t_final), L.ptr(last_ids), L.ptr(tile_cost), None, None, 0, st), "fwd")


def backward():
    L.check(lib.qed_composite_bwd(1, n, L.ptr(splats), L.ptr(ids), L.ptr(offsets), w, h, tw, th, 3, None, L.ptr(alpha),
                                  L.ptr(t_final), L.ptr(last_ids), L.ptr(v_render), L.ptr(v_alpha), L.ptr(vsplat),
                                  L.ptr(tile_cost), L.ptr(order_ws), None, 0, st), "bwd")


def contribution():
    scores.add_view(info, 1, n, w, h, launch_flags=0)


def timed(fn, before=None):
    ms = []
    for it in range(iters + 3):
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


result = {"gaussians": n, "width": w, "height": h, "iters": iters}
result["composite_fwd"] = timed(forward)
result["contribution"] = timed(contribution)
result["contribution_zeroed_each_time"] = timed(contribution, before=lambda: scores.zero_())
result["composite_bwd_unit_gradient"] = timed(backward, before=lambda: vsplat.zero_())
runs = torch.diff(offsets[: tw * th + 1].to(torch.int64))
scores.zero_()
contribution()
torch.cuda.synchronize()
result["list_length"] = int(runs.sum())
result["batches_of_64"] = int(((runs + 63) // 64).sum())
result["atomic_wave_instructions_upper_bound"] = 3 * result["batches_of_64"]
result["one_lane_per_gaussian_form_upper_bound"] = 3 * result["list_length"]
result["gaussians_scored_above_zero"] = int((scores.hits() > 0).sum())
result["gaussians_max_weight_at_least_0.01"] = int((scores.max_weight() >= 0.01).sum())
# the backward's colour column is the other route to the sum: the two agree
rel = (vsplat[:, 8].double() - scores.sum_weight()).abs().max() / scores.sum_weight().max()
result["sum_weight_vs_backward_column_max_rel"] = float(rel)
print(json.dumps(result))
