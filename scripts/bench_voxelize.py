"""Reconstruction-output timing: nlosgr.voxelize (HIP) on the C3 synthetic model (100k Gaussians, cuda
preset, SH degree 3) onto 256^3 and 64^3 voxels at cutoffs 3 and 5.7, and, at 64^3 only, what a user could
do before nlosgr.voxelize existed: a chunked torch-on-GPU evaluation of the same masked sums (materialised
[chunk, Nvox] tensors, written below).  The torch route is not run at 256^3: 1.7e12 evaluations through
materialised chunks.  Warm-up, timed repeats, device-event timing (as bench.py); writes one JSON file.

    python scripts/bench_voxelize.py [--out profiles/voxelize_c3.json] [--ng 100000] [--repeats 5]
    python scripts/bench_voxelize.py --kernel-stats STATS.csv   # embed a rocprofv3 --kernel-trace --stats
                                                                # summary of `--profile-run` as the phase split
    python scripts/bench_voxelize.py --profile-run              # two 256^3 cutoff-3 calls, for the profiler
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nlosgr  # noqa: E402
from nlosgr.voxelize import VoxelGrid, voxelize  # noqa: E402

DEV = torch.device("cuda:0")
CAM = (0.0, 0.0, 0.0)
POS, SIZE = (0.0, 0.5, 0.0), 0.5


def timed(fn, warmup, repeats):
    """Per-call milliseconds (device events around each call), after `warmup` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "repeats": len(s)}


@torch.no_grad()
def torch_route(model, grid, cam, cutoff, chunk):
    """The same sums in plain torch (cuda preset conventions, cuda_utils.cuh:54-151): Gaussians in chunks of
    `chunk`, each chunk a dense [chunk, Nvox] broadcast, masked at m^2 <= cutoff^2."""
    x = grid.coords().reshape(-1, 3).to(DEV)                                        # [Nv, 3]
    mu, S, Q, O = model._mu, model._scaling, model._rotation, model._opacity.reshape(-1)
    f = nlosgr.features_flat(model)
    n = Q.norm(dim=1, keepdim=True)
    w, a, b, c = (Q / n).unbind(1)
    R = torch.stack([1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b),
                     2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a),
                     2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)], dim=1).reshape(-1, 3, 3)
    A = R.transpose(1, 2) / (torch.exp(S) + 1e-8).unsqueeze(-1)                     # u = A (x - mu)
    d = mu - cam
    d = d / (d.norm(dim=1, keepdim=True) + 1e-8)
    from oracle.torch_ref import eval_sh_cuda
    rho = torch.clamp_min(eval_sh_cuda(model.active_sh_degree, f, d) + 0.5, 0.0)
    sig = torch.sigmoid(O)
    dens = torch.zeros(x.shape[0], device=DEV)
    alb = torch.zeros(x.shape[0], device=DEV)
    for i in range(0, mu.shape[0], chunk):
        j = min(i + chunk, mu.shape[0])
        u = torch.einsum("grc,gvc->gvr", A[i:j], x.unsqueeze(0) - mu[i:j].unsqueeze(1))   # [chunk, Nv, 3]
        m2 = (u * u).sum(-1)
        pdf = torch.exp(-0.5 * m2)
        if cutoff > 0:
            pdf = torch.where(m2 <= cutoff * cutoff, pdf, torch.zeros_like(pdf))
        dens += sig[i:j] @ pdf
        alb += (sig[i:j] * rho[i:j]) @ pdf
    return dens.reshape(grid.shape), alb.reshape(grid.shape)


def kernel_stats(path):
    """{kernel family: total ns, calls} of this library's voxel kernels from a rocprofv3 stats CSV."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            for fam in ("preprocess_kernel", "voxel_aux_kernel", "voxel_bin_kernel", "voxel_eval_kernel"):
                if fam in name:
                    e = out.setdefault(fam, {"calls": 0, "total_ms": 0.0})
                    e["calls"] += int(float(row["Calls"]))
                    e["total_ms"] += float(row["TotalDurationNs"]) / 1e6
    for e in out.values():
        e["ms_per_call"] = e["total_ms"] / max(e["calls"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelize_c3.json"))
    ap.add_argument("--ng", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=256, help="Gaussians per torch chunk at 64^3 (3 GiB of [chunk, Nvox, 3])")
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voxelize needs a GPU"
    model = nlosgr.GaussianParams.synthetic(a.ng, 3, preset="cuda", device=DEV, seed=0)
    cam = torch.tensor(CAM, device=DEV)
    big, small = VoxelGrid(POS, SIZE, 256), VoxelGrid(POS, SIZE, 64)
    if a.profile_run:
        for _ in range(2):
            voxelize(model, big, cam, preset="cuda", cutoff=3.0)
        torch.cuda.synchronize()
        return
    res = {"workload": f"C3 synthetic model: {a.ng} Gaussians, cuda preset, SH degree 3, seed 0; volume {SIZE} at {POS}",
           "device": torch.cuda.get_device_name(0), "timing": "device events around each call, median of repeats",
           "hip": {}, "torch_chunked_64": {}}
    for name, grid in (("256", big), ("64", small)):
        for cutoff in (3.0, 5.7):
            ms = timed(lambda: voxelize(model, grid, cam, preset="cuda", cutoff=cutoff), a.warmup, a.repeats)
            res["hip"][f"{name}^3 cutoff {cutoff}"] = stats(ms)
            print(name, cutoff, res["hip"][f"{name}^3 cutoff {cutoff}"], flush=True)
    for cutoff in (3.0, 5.7):
        ms = timed(lambda: torch_route(model, small, cam, cutoff, a.torch_chunk), 1, 2)
        key = f"64^3 cutoff {cutoff}"
        res["torch_chunked_64"][key] = dict(stats(ms), chunk=a.torch_chunk)
        hd, ha = voxelize(model, small, cam, preset="cuda", cutoff=cutoff)
        td, ta = torch_route(model, small, cam, cutoff, a.torch_chunk)
        res["torch_chunked_64"][key]["rel_l2_vs_hip"] = {
            "density": ((hd - td).double().norm() / td.double().norm()).item(),
            "albedo": ((ha - ta).double().norm() / ta.double().norm()).item()}
        res["torch_chunked_64"][key]["speedup_hip"] = (res["torch_chunked_64"][key]["median_ms"] /
                                                       res["hip"][key]["median_ms"])
        print("torch", cutoff, res["torch_chunked_64"][key], flush=True)
    res["torch_256"] = "not run: 1.7e12 evaluations through materialised [chunk, Nvox] tensors"
    if a.kernel_stats:
        res["kernel_split_256_cutoff_3"] = kernel_stats(a.kernel_stats)
        res["kernel_split_note"] = ("rocprofv3 --kernel-trace --stats of --profile-run (separate run): voxel_bin_kernel is "
                                    "level-1 binning; voxel_eval_kernel holds level-2 culling and evaluation together")
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": "voxelize 64^3 cutoff 3: torch chunked / HIP", "value":
                      res["torch_chunked_64"]["64^3 cutoff 3.0"]["speedup_hip"]}))


if __name__ == "__main__":
    main()
