#!/usr/bin/env python3
"""What the depth spread and the depth distortion term cost (csrc/depth_spread.hip, depth_distortion.py), at config B
(500 000 Gaussians, 1920x1080) unless sizes are given.  HIP events around each call, median / min over the iterations.

  kernels     qed_depth_spread_fwd against qed_composite_fwd (4 channels) and qed_contribution on the same lists;
              qed_depth_spread_bwd against qed_composite_bwd (4 channels); qed_depth_distortion_loss
  two-pass    the route not taken: qed_composite_fwd + qed_composite_bwd (3 channels) of the unchanged compositing kernels with
              (z, z^2, 0) in the colour slots -- its time, and on a THIN depth setting (the scene's depths mapped to 4 +- 0.02)
              how far the loss and the per-pixel spread it forms from raw float32 moments, A D2 - D^2, lie from the Welford
              kernel's (which tests/test_depth_spread.py holds to the float64 oracle)
  step        one training step on both routes with depth_distortion_lambda 0.1 against the same step with lambda 0
  bench       with --parent DIR (a checkout of the parent commit with its library built): bench.py there and here, a fresh
              process each, alternating

    python scripts/bench_depth_distortion.py [--iters 30] [--gaussians N --width W --height H]
                                             [--parent DIR [--bench-rounds 4 --bench-steps 300]] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from qed_splatter_amd import _lib as L  # noqa: E402
from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig, get_viewmat  # noqa: E402
from qed_splatter_amd.prune import ContributionScores  # noqa: E402
from qed_splatter_amd.rasterization import rasterization  # noqa: E402
from qed_splatter_amd.scene import synthetic_scene  # noqa: E402

PARAMS = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


def timed(fn, iters, before=None):
    us = []
    for it in range(iters + 3):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= 3:
            us.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1)}


def bench_value(tree, steps, warmup):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                         cwd=tree, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"bench.py failed in {tree}:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return float(json.loads(out.stdout.strip().splitlines()[-1])["value"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parent", default=None, metavar="DIR")
    ap.add_argument("--bench-rounds", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--out", default=None, metavar="FILE")
    a = ap.parse_args()
    n, w, h, iters = a.gaussians, a.width, a.height, a.iters
    dev = torch.device("cuda:0")
    lib = L.load()
    sc = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in synthetic_scene(n, w, h, seed=1235).items()}
    with torch.no_grad():
        _, _, info = rasterization(
            means=sc["means"], quats=torch.nn.functional.normalize(sc["quats"], dim=-1), scales=sc["scales"].exp(),
            opacities=torch.sigmoid(sc["opacities"]).squeeze(-1),
            colors=torch.cat([sc["features_dc"][:, None, :], sc["features_rest"]], dim=1),
            viewmats=get_viewmat(sc["camera_to_worlds"][:1]), Ks=sc["Ks"][:1], width=w, height=h, render_mode="RGB+D",
            sh_degree=3, _keep_records=True)
    splats, ids, offsets = info["_splats"], info["flatten_ids"], info["_isect_offsets_full"]
    tw, th = info["tile_width"], info["tile_height"]
    st = L.current_stream()
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    render4, render3, alpha, t_final = f32(1, h, w, 4), f32(1, h, w, 3), f32(1, h, w, 1), f32(1, h, w)
    last_ids = torch.empty(1, h, w, dtype=torch.int32, device=dev)
    tile_cost = torch.empty(tw * th, 4, dtype=torch.int32, device=dev)
    order_ws = torch.empty(tw * th + 1, dtype=torch.int32, device=dev)
    planes = f32(4, 1, h, w)
    v = torch.full((1, h, w), 1.0 / (h * w), device=dev)
    rows = torch.zeros(n, L.VSPLAT_FLOATS, device=dev)
    ws = torch.empty(L.DEPTH_DISTORTION_WS_DOUBLES, dtype=torch.float64, device=dev)
    loss = f32(1)
    scores = ContributionScores(n, dev)

    def comp_fwd(records, channels, render):
        L.check(lib.qed_composite_fwd(1, n, L.ptr(records), L.ptr(ids), L.ptr(offsets), w, h, tw, th, channels, None,
                                      L.ptr(render), L.ptr(alpha), L.ptr(t_final), L.ptr(last_ids), L.ptr(tile_cost), None,
                                      None, 0, st), "fwd")

    def comp_bwd(records, channels, v_render):
        L.check(lib.qed_composite_bwd(1, n, L.ptr(records), L.ptr(ids), L.ptr(offsets), w, h, tw, th, channels, None,
                                      L.ptr(alpha), L.ptr(t_final), L.ptr(last_ids), L.ptr(v_render), L.ptr(v_alpha),
                                      L.ptr(rows), L.ptr(tile_cost), L.ptr(order_ws), None, 0, st), "bwd")

    def spread_fwd(records):
        L.check(lib.qed_depth_spread_fwd(1, n, L.ptr(records), L.ptr(ids), L.ptr(offsets), w, h, tw, th, L.ptr(planes[0]),
                                         L.ptr(planes[1]), L.ptr(planes[2]), L.ptr(planes[3]), 0, st), "spread fwd")

    def spread_bwd(records):
        L.check(lib.qed_depth_spread_bwd(1, n, L.ptr(records), L.ptr(ids), L.ptr(offsets), w, h, tw, th, L.ptr(t_final),
                                         L.ptr(last_ids), L.ptr(planes[0]), L.ptr(planes[1]), L.ptr(planes[2]), L.ptr(v),
                                         L.ptr(rows), L.ptr(tile_cost), L.ptr(order_ws), 0, st), "spread bwd")

    def dist_loss():
        L.check(lib.qed_depth_distortion_loss(h * w, L.ptr(planes[0]), None, 0.1, L.ptr(ws), L.ptr(v), L.ptr(loss), st), "loss")

    v_alpha = torch.zeros(1, h, w, 1, device=dev)
    v4, v3 = torch.ones(1, h, w, 4, device=dev), torch.ones(1, h, w, 3, device=dev)
    res = {"gaussians": n, "width": w, "height": h, "iters": iters,
           "list_length": int(torch.diff(offsets[: tw * th + 1].to(torch.int64)).sum())}
    # ---- kernels ----
    comp_fwd(splats, 4, render4)
    res["composite_fwd_4ch"] = timed(lambda: comp_fwd(splats, 4, render4), iters)
    res["contribution"] = timed(lambda: scores.add_view(info, 1, n, w, h, launch_flags=0), iters)
    res["depth_spread_fwd"] = timed(lambda: spread_fwd(splats), iters)
    res["composite_bwd_4ch"] = timed(lambda: comp_bwd(splats, 4, v4), iters, before=lambda: rows.zero_())
    res["depth_spread_bwd"] = timed(lambda: spread_bwd(splats), iters, before=lambda: rows.zero_())
    res["depth_distortion_loss"] = timed(dist_loss, iters)
    # ---- the route not taken: (z, z^2, 0) through the unchanged compositing kernels ----
    z = splats.view(-1, L.SPLAT_FLOATS)[:, 9]
    seen = z > 0
    zmin, zmax = float(z[seen].min()), float(z[seen].max())
    thin = splats.clone()
    zt = torch.where(seen, 4.0 + 0.04 * ((z - zmin) / (zmax - zmin) - 0.5), z)
    thin.view(-1, L.SPLAT_FLOATS)[:, 9] = zt
    moments = thin.clone()
    mv = moments.view(-1, L.SPLAT_FLOATS)
    mv[:, 6], mv[:, 7], mv[:, 8] = zt, zt * zt, 0.0
    res["two_pass_fwd_3ch"] = timed(lambda: comp_fwd(moments, 3, render3), iters)
    res["two_pass_bwd_3ch"] = timed(lambda: comp_bwd(moments, 3, v3), iters, before=lambda: rows.zero_())
    comp_fwd(moments, 3, render3)
    spread_fwd(thin)
    torch.cuda.synchronize()
    A, D, D2 = alpha[0, ..., 0].double(), render3[0, ..., 0].double(), render3[0, ..., 1].double()
    raw = (alpha[0, ..., 0] * render3[0, ..., 1] - render3[0, ..., 0] * render3[0, ..., 0]).double()     # float32 arithmetic
    raw64 = A * D2 - D * D                              # the float32 moments, combined in double
    good = planes[0, 0].double()
    covered = good > 1e-3 * float(good.max())
    rel = lambda x: ((x - good).abs() / good)[covered]
    res["thin_setting"] = {
        "depth_range": [float(zt[seen].min()), float(zt[seen].max())],
        "loss_welford": float(good.mean()), "loss_raw_moments_f32": float(raw.mean()),
        "loss_raw_moments_combined_in_f64": float(raw64.mean()),
        "loss_rel_err_raw_f32": abs(float(raw.mean()) - float(good.mean())) / float(good.mean()),
        "loss_rel_err_raw_combined_in_f64": abs(float(raw64.mean()) - float(good.mean())) / float(good.mean()),
        "pixel_rel_err_raw_f32_median": float(rel(raw).median()), "pixel_rel_err_raw_f32_p99": float(rel(raw).quantile(0.99)),
        "pixel_rel_err_raw_f64comb_median": float(rel(raw64).median()),
        "pixel_rel_err_raw_f64comb_p99": float(rel(raw64).quantile(0.99)), "covered_pixels": int(covered.sum())}
    # ---- a training step on both routes, lambda 0.1 against lambda 0 ----
    K = sc["Ks"][0]
    cam = PinholeCameras(sc["camera_to_worlds"][:1], float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), w, h,
                         metadata={"cam_idx": 0})
    batch = {"image": sc["gt_rgb"] if "gt_rgb" in sc else torch.rand(h, w, 3, device=dev),
             "depth_image": torch.full((h, w, 1), 3.0, device=dev)}
    steps = {}
    for lam in (0.0, 0.1):
        m = QEDSplatterModel(QEDSplatterModelConfig.synthetic(depth_distortion_lambda=lam, graph_segments=False),
                             **{k: sc[k] for k in PARAMS})
        m.step = 100000
        m.train()

        def fused():
            for p in m.parameters():
                p.grad = None
            m.backward_fused(m.fused_loss(cam, batch))

        def api():
            for p in m.parameters():
                p.grad = None
            sum(m.get_loss_dict(m.get_outputs(cam), batch).values()).backward()
        steps[f"fused_lambda_{lam}"] = timed(fused, iters)
        steps[f"api_lambda_{lam}"] = timed(api, iters)
    res["step"] = steps
    # ---- bench.py here and in the parent, alternating ----
    if a.parent:
        here_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        there, here = [], []
        for _ in range(a.bench_rounds):
            there.append(bench_value(a.parent, a.bench_steps, 50))
            here.append(bench_value(here_dir, a.bench_steps, 50))
        res["bench_parent_iters_per_s"], res["bench_here_iters_per_s"] = there, here
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
