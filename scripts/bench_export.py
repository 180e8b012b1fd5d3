#!/usr/bin/env python3
"""Exporting trained Gaussians as a 3DGS PLY file (qed_splatter_amd/gaussian_ply.py, csrc/export.hip) at 500 k and 5 M
Gaussians of SH degree 3 (248 bytes per row), 1 % of the rows planted non-finite or transparent.  Three things are timed,
each as the median of the runs after warm-up:
  pack      the three launches of qed_pack_gaussians alone (device events);
  export    export_gaussian_ply to a file on /dev/shm: pack + the copy of the count words + ONE device-to-host copy of the
            rows kept + the file write (wall clock around the call, device idle before and after);
  host      the same export done the way ns-export gaussian-splat does it on the host, from the same device tensors
            (tests/gaussian_ply_ref.py::nerfstudio_style_export): a .cpu().numpy() per attribute, an isfinite pass per
            property, two boolean filters, a structured-array fill per property -- the baseline.
The two files are compared byte for byte once.  Its output is the first section of profiles/export.txt.

    python scripts/bench_export.py [--sizes 500000 5000000 --runs 10 --host-runs 3] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from qed_splatter_amd import gaussian_ply as G  # noqa: E402
from tests import gaussian_ply_ref as ref  # noqa: E402

COPY_TBS = 5.42          # profiles/r01_hbm_copy_bench.txt: copy 1 GiB -> 1 GiB, read + write


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def make_model(n, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    p = {"means": torch.randn(n, 3, device=dev, generator=g) * 3, "scales": torch.rand(n, 3, device=dev, generator=g) * 5 - 6,
         "quats": torch.randn(n, 4, device=dev, generator=g), "opacities": torch.rand(n, 1, device=dev, generator=g) * 10 - 4,
         "features_dc": torch.rand(n, 3, device=dev, generator=g) * 3 - 1.5,
         "features_rest": torch.randn(n, 15, 3, device=dev, generator=g) * 0.3}
    bad = torch.rand(n, device=dev, generator=g)
    p["features_rest"][bad < 0.005, 7, 1] = float("nan")
    p["opacities"][(bad >= 0.005) & (bad < 0.01)] = -8.0
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[500_000, 5_000_000])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--host-runs", type=int, default=3, help="runs of the host baseline (it takes seconds at 5 M)")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_export.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    say("# exporting Gaussians of SH degree 3 (248 B per row) as a 3DGS PLY file; 1 % of the rows dropped")
    say(f"# commit {commit or '(not a git checkout)'}; {torch.cuda.get_device_name(0)}; torch {torch.__version__}; medians of "
        f"{args.runs} runs after 3 warm-up runs (host baseline: {args.host_runs} runs after 1); files on {tmp}")
    say("# pack: bytes = parameters read twice (count pass, pack pass) + rows written; 'of copy' = that rate over the "
        f"{COPY_TBS} TB/s of profiles/r01_hbm_copy_bench.txt")
    say("# Gaussians   kept      pack ms   pack GB/s  of copy   export ms (file MB)   host-route ms   host / export")
    results = []
    for n in args.sizes:
        p = make_model(n, dev)
        path, path_ref = os.path.join(tmp, "splat.ply"), os.path.join(tmp, "splat_ref.ply")
        pack_ms = []
        for i in range(args.runs + 3):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rows, counts = G.pack_gaussians(p, 3)
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                pack_ms.append(a.elapsed_time(b))
            del rows
        kept = int(counts[0])
        export_ms = []
        for i in range(args.runs + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = G.export_gaussian_ply(p, path)
            torch.cuda.synchronize()
            if i >= 3:
                export_ms.append(1e3 * (time.perf_counter() - t0))
        assert res["written"] == kept
        host_ms = []
        if not args.skip_host:
            for i in range(args.host_runs + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                count = ref.nerfstudio_style_export(p, path_ref, 3)
                if i >= 1:
                    host_ms.append(1e3 * (time.perf_counter() - t0))
            assert count == kept
            with open(path, "rb") as f1, open(path_ref, "rb") as f2:
                assert f1.read() == f2.read(), "the two routes wrote different files"
        moved = 2 * n * 59 * 4 + kept * 248
        pm, em = median(pack_ms), median(export_ms)
        hm = median(host_ms) if host_ms else float("nan")
        rate = moved / (pm * 1e-3)
        say(f"{n:10d}  {kept:9d}  {pm:8.3f}   {rate / 1e9:8.1f}   {100 * rate / (COPY_TBS * 1e12):5.1f} %   {em:9.1f} "
            f"({os.path.getsize(path) / 1e6:7.1f})   {hm:12.1f}   {hm / em:10.1f}")
        results.append({"gaussians": n, "kept": kept, "pack_ms": pm, "pack_gbs": rate / 1e9, "export_ms": em, "host_ms": hm})
        for f in (path, path_ref):
            if os.path.exists(f):
                os.remove(f)
        del p
        torch.cuda.empty_cache()
    os.rmdir(tmp)
    print(json.dumps(results))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
