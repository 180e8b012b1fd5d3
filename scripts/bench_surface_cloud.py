#!/usr/bin/env python3
"""The surface-cloud export at config B's scene (500 k Gaussians, 1920 x 1080; qed_splatter_amd/surface_cloud.py,
csrc/surface.hip, csrc/voxel.hip).  Timed with device events, each as the median of the runs after warm-up:
  samples   qed_surface_samples on one rendered view (every filter on) beside the same result made with torch statements
            on the same device (masks, boolean gathers over the planes, float64 arithmetic); the two alternate;
  voxels    qed_voxel_down_sample_attr on that view's samples (6 attribute columns, weights given) beside torch.unique +
            index_add_ in float64;
  export    the whole export_pointcloud over the synthetic scene's cameras (render, samples, merge, finish), no file.
Bytes over kernel time are counted from the shapes: the planes the launch has to read once and the rows it writes.
Its output is profiles/surface_cloud.txt.

    python scripts/bench_surface_cloud.py [--runs 20] [--cameras 8] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sc -- python scripts/bench_surface_cloud.py --trace-only 20
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from qed_splatter_amd import surface_cloud as SC  # noqa: E402
from qed_splatter_amd.model import PinholeCameras, QEDSplatterModel, QEDSplatterModelConfig  # noqa: E402
from qed_splatter_amd.scene import synthetic_scene  # noqa: E402

COPY_TBS = 5.42          # profiles/r01_hbm_copy_bench.txt: copy 1 GiB -> 1 GiB, read + write
W, H, N = 1920, 1080, 500_000
FILTERS = dict(min_alpha=0.5, depth_min=0.0, depth_max=1e4, max_normal_angle_deg=60.0, min_view_cos=0.1)
VOXEL = 0.01


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(fn, runs, warmup):
    ms = []
    for i in range(runs + warmup):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


def torch_samples(o, viewmat, intr):
    """The definition of qed_surface_samples with torch statements (float64 where the kernel is)."""
    fx, fy, cx, cy = intr
    a, d = o["accumulation"][..., 0], o["depth"][..., 0]
    nr, nd, bits = o["normal"], o["depth_normal"], o["normal_valid"]
    keep = a >= FILTERS["min_alpha"]
    z = d.double() / a.double()
    keep &= torch.isfinite(z) & (z >= FILTERS["depth_min"]) & (z <= FILTERS["depth_max"])
    keep &= (bits & 1) != 0
    dot = (nr.double() * nd.double()).sum(-1)
    keep &= ((bits & 3) != 3) | (dot >= SC.cos_max_normal_angle(FILTERS["max_normal_angle_deg"]))
    xs = (torch.arange(W, device=z.device, dtype=torch.float64) + 0.5 - cx) / fx
    ys = (torch.arange(H, device=z.device, dtype=torch.float64) + 0.5 - cy) / fy
    P = torch.stack([xs[None, :] * z, ys[:, None] * z, z], dim=-1)
    view = P / P.norm(dim=-1, keepdim=True)
    keep &= -(nr.double() * view).sum(-1) >= FILTERS["min_view_cos"]
    R, t = viewmat[:3, :3].double(), viewmat[:3, 3].double()
    pts = ((P[keep] - t) @ R).float()
    nrm = (nr[keep].double() @ R).float()
    return pts, nrm, o["rgb"][keep]


def torch_voxels(points, attrs, weights, v):
    # (a device tensor as divisor: torch turns a division by a host scalar into a multiplication by its reciprocal, which
    #  moves points that sit on a voxel border)
    keys = torch.floor(points / torch.full((), v, dtype=points.dtype, device=points.device)).to(torch.int64)
    keys = keys - keys.min(dim=0).values
    span = keys.max(dim=0).values + 1
    flat = (keys[:, 0] * span[1] + keys[:, 1]) * span[2] + keys[:, 2]
    _, inv = torch.unique(flat, return_inverse=True)
    m = int(inv.max()) + 1
    w = weights.double()
    cols = torch.cat([points.double(), attrs.double(), torch.ones_like(w)[:, None]], dim=1) * w[:, None]
    out = torch.zeros(m, cols.shape[1], dtype=torch.float64, device=points.device)
    out.index_add_(0, inv, cols)
    return (out[:, :-1] / out[:, -1:]).float(), out[:, -1].float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--trace-only", type=int, default=0, metavar="N", help="N rounds of the two hip calls and nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_cloud.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sc = synthetic_scene(N, W, H, 7, n_cameras=args.cameras)
    d = {k: sc[k].to(dev) for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest")}
    K = sc["Ks"][0]
    intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    model = QEDSplatterModel(QEDSplatterModelConfig.synthetic(output_normals=True), **d)
    model.step = 10_000
    model.eval()
    cams = [PinholeCameras(sc["camera_to_worlds"][k:k + 1].to(dev), *intr, W, H) for k in range(args.cameras)]
    with torch.no_grad():
        o = model.get_outputs(cams[0])
    viewmat = SC.camera_viewmat(cams[0], dev)
    planes = (o["rgb"], o["depth"], o["accumulation"], o["normal"], o["depth_normal"], o["normal_valid"], viewmat, intr)
    state = {}

    def k_samples():
        state["s"] = SC.surface_samples(*planes, **FILTERS)

    k_samples()
    pts, nrm, col = state["s"]
    n = int(pts.shape[0])
    attrs = torch.cat([nrm, col], dim=1).contiguous()
    weights = torch.rand(n, device=dev) * 3.0 + 0.5

    def k_voxels():
        state["v"] = SC.voxel_down_sample_attr(pts, attrs, weights, VOXEL)

    if args.trace_only:
        for _ in range(args.trace_only):
            k_samples(); k_voxels()
        torch.cuda.synchronize()
        return

    tstate = {}

    def t_samples():
        tstate["s"] = torch_samples(o, viewmat, intr)

    def t_voxels():
        tstate["v"] = torch_voxels(pts, attrs, weights, VOXEL)

    k_voxels(); t_samples(); t_voxels()
    say(f"# the surface-cloud export at {N} Gaussians, {W} x {H} (config B's scene, seed 7): {n} of {W * H} pixels of view 0 "
        f"kept, {int(state['v'][0].shape[0])} voxels of {VOXEL}")
    say(f"# MI355X ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}); torch {torch.__version__}; device events "
        f"around each call (its host read of the count included); medians of {args.runs} runs after 3 warm-up runs; hip and "
        "torch alternate")
    res = {}
    say("# call / statement group                                    median ms      min ms      max ms")
    for hn, hf, tn, tf in (("surface_samples (3 launches)", k_samples, "masks + boolean gathers, float64", t_samples),
                           ("voxel_down_sample_attr, K = 6", k_voxels, "unique + index_add_, float64", t_voxels)):
        hm, tm = [], []
        timed(hf, 0, 3); timed(tf, 0, 2)
        for _ in range(args.runs):
            hm += timed(hf, 1, 0)
            tm += timed(tf, 1, 0)
        say(f"hip    {hn:50s} {median(hm):10.4f}  {min(hm):10.4f}  {max(hm):10.4f}")
        say(f"torch  {tn:50s} {median(tm):10.4f}  {min(tm):10.4f}  {max(tm):10.4f}   torch / hip {median(tm) / median(hm):.1f} x")
        res[hn] = median(hm)
        res["torch: " + tn] = median(tm)
    n_pix = W * H
    need = n_pix * 9 + n * (8 + 24 + 36)
    say(f"bytes qed_surface_samples has to move for this view: {need / 1e6:.1f} MB = {n_pix} pixels x 9 B (alpha, depth, valid) "
        f"+ {n} kept x (8 B alpha and depth again + 24 B colour and normal + 36 B out); with the agreement or the grazing filter "
        f"on, the deciding launch also reads 24 B of normals per pixel that passed the tests before them.  Over the kernel times "
        f"of the trace this is the share of the {COPY_TBS} TB/s copy rate of profiles/r01_hbm_copy_bench.txt quoted below.")
    dp = float((state["s"][0] - tstate["s"][0]).abs().max()) if tstate["s"][0].shape == state["s"][0].shape else float("nan")
    dv = float((state["v"][0] - tstate["v"][0][:, :3]).abs().max()) if tstate["v"][0].shape[0] == state["v"][0].shape[0] else float("nan")
    say(f"largest difference between the two routes: sample positions {dp:.3g}, voxel means {dv:.3g} "
        f"({int(state['v'][0].shape[0])} and {int(tstate['v'][0].shape[0])} voxels)")

    # ---- the whole export ----
    ms = []
    for i in range(5):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        cloud = SC.export_pointcloud(model, cams, voxel_size=VOXEL, **{k: v for k, v in FILTERS.items()})
        b.record()
        torch.cuda.synchronize()
        if i >= 1:
            ms.append(a.elapsed_time(b))
    say(f"export_pointcloud over {args.cameras} cameras (render + samples + merge + finish, no file): median {median(ms):.2f} ms "
        f"(min {min(ms):.2f}, max {max(ms):.2f}) = {median(ms) / args.cameras:.2f} ms per view; {len(cloud)} points")
    res.update({"export_ms": median(ms), "kept": n, "need_bytes": need, "points": len(cloud)})
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
