"""Voxelizer-backward timing: nlosgr.voxelize.voxelize_backward (HIP) beside the forward and one VoxelFitStep step
(volume mode) on the C3 synthetic model (100k Gaussians, cuda preset, SH degree 3) onto 128^3 and 256^3 voxels at
cutoff 3, and, at a size its dense [Ng, Nvox] tensors fit (2,000 Gaussians x 64^3), what a user could do before
nlosgr_voxelize_bwd existed: the torch-autograd composition of the same formula on the GPU in fp32, written below
(forward + backward: autograd has no backward without its forward).  Warm-up, timed repeats, device-event timing
(as scripts/bench_voxelize.py); writes one JSON file.

    python scripts/bench_voxelize_bwd.py [--out profiles/voxelize_bwd_c3.json] [--ng 100000] [--repeats 5]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nlosgr  # noqa: E402
from nlosgr.voxel_fit import VoxelFitStep  # noqa: E402
from nlosgr.voxelize import VoxelGrid, voxelize, voxelize_backward  # noqa: E402

DEV = torch.device("cuda:0")
CAM = (0.0, 0.0, 0.0)
POS, SIZE = (0.0, 0.5, 0.0), 0.5
CUTOFF = 3.0


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


def torch_composition(model, grid, cam, cutoff, gd, ga):
    """(d_mu, d_scaling, d_rotation, d_opacity, d_features) by torch autograd through the dense [Ng, Nvox] evaluation
    of the two sums (cuda preset conventions, cuda_utils.cuh:54-151), masked at m^2 <= cutoff^2."""
    from oracle.torch_ref import eval_sh_cuda
    x = grid.coords().reshape(-1, 3).to(DEV)
    mu, S, Q, O, f = [t.detach().clone().requires_grad_(True) for t in
                      (model._mu, model._scaling, model._rotation, model._opacity.reshape(-1),
                       nlosgr.features_flat(model))]
    w, a, b, c = (Q / Q.norm(dim=1, keepdim=True)).unbind(1)
    R = torch.stack([1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b),
                     2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a),
                     2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)], dim=1).reshape(-1, 3, 3)
    A = R.transpose(1, 2) / (torch.exp(S) + 1e-8).unsqueeze(-1)
    d = mu - cam
    d = d / (d.norm(dim=1, keepdim=True) + 1e-8)
    rho = torch.clamp_min(eval_sh_cuda(model.active_sh_degree, f, d) + 0.5, 0.0)
    sig = torch.sigmoid(O)
    u = torch.einsum("grc,gvc->gvr", A, x.unsqueeze(0) - mu.unsqueeze(1))
    m2 = (u * u).sum(-1)
    pdf = torch.exp(-0.5 * m2)
    if cutoff > 0:
        pdf = torch.where(m2 <= cutoff * cutoff, pdf, torch.zeros_like(pdf))
    L = ((sig @ pdf) * gd.reshape(-1)).sum() + (((sig * rho) @ pdf) * ga.reshape(-1)).sum()
    L.backward()
    return mu.grad, S.grad, Q.grad, O.grad, f.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelize_bwd_c3.json"))
    ap.add_argument("--ng", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--torch-ng", type=int, default=2000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_voxelize_bwd needs a GPU"
    model = nlosgr.GaussianParams.synthetic(a.ng, 3, preset="cuda", device=DEV, seed=0)
    cam = torch.tensor(CAM, device=DEV)
    gen = torch.Generator(device="cpu").manual_seed(1)
    res = {"workload": f"C3 synthetic model: {a.ng} Gaussians, cuda preset, SH degree 3, seed 0; volume {SIZE} at {POS}; "
                       f"cutoff {CUTOFF}; both outputs / both upstreams (seeded normal noise)",
           "device": torch.cuda.get_device_name(0), "timing": "device events around each call, median of repeats",
           "hip": {}}
    for n in (128, 256):
        grid = VoxelGrid(POS, SIZE, n)
        gd, ga = torch.randn(grid.shape, generator=gen).to(DEV), torch.randn(grid.shape, generator=gen).to(DEV)
        kw = dict(preset="cuda", cutoff=CUTOFF)
        fwd = stats(timed(lambda: voxelize(model, grid, cam, **kw), a.warmup, a.repeats))
        bwd = stats(timed(lambda: voxelize_backward(model, grid, cam, gd, ga, **kw), a.warmup, a.repeats))
        fit_model = nlosgr.GaussianParams.synthetic(a.ng, 3, preset="cuda", device=DEV, seed=0)
        step = VoxelFitStep(fit_model, grid, cam, target_volume=ga.abs(), **kw)
        fit = stats(timed(step, a.warmup, a.repeats))
        res["hip"][f"{n}^3"] = {"voxelize": fwd, "voxelize_backward": bwd, "voxel_fit_step_volume_mode": fit,
                                "backward_over_forward": bwd["median_ms"] / fwd["median_ms"]}
        if n == 128:
            # boxes are not cut: one wave walks a grid-covering Gaussian alone (nvox / 64 steps).  What one costs:
            wide = nlosgr.GaussianParams.synthetic(a.ng, 3, preset="cuda", device=DEV, seed=0)
            wide._mu.data[0] = torch.tensor(POS, device=DEV)
            wide._scaling.data[0] = math.log(SIZE)
            one = stats(timed(lambda: voxelize_backward(wide, grid, cam, gd, ga, **kw), a.warmup, a.repeats))
            res["hip"][f"{n}^3"]["voxelize_backward_with_one_grid_covering_gaussian"] = one
            del wide
        print(n, res["hip"][f"{n}^3"], flush=True)
        del gd, ga, step, fit_model
    # against torch autograd, where its dense tensors fit
    small = nlosgr.GaussianParams.synthetic(a.torch_ng, 3, preset="cuda", device=DEV, seed=0)
    grid = VoxelGrid(POS, SIZE, 64)
    gd, ga = torch.randn(grid.shape, generator=gen).to(DEV), torch.randn(grid.shape, generator=gen).to(DEV)
    kw = dict(preset="cuda", cutoff=CUTOFF)
    hip_b = stats(timed(lambda: voxelize_backward(small, grid, cam, gd, ga, **kw), a.warmup, a.repeats))
    hip_f = stats(timed(lambda: voxelize(small, grid, cam, **kw), a.warmup, a.repeats))
    tor = stats(timed(lambda: torch_composition(small, grid, cam, CUTOFF, gd, ga), 1, 3))
    got = voxelize_backward(small, grid, cam, gd, ga, **kw)
    ref = torch_composition(small, grid, cam, CUTOFF, gd, ga)
    names = ("d_mu", "d_scaling", "d_rotation", "d_opacity", "d_features")
    rel = {k: ((g.reshape(-1) - r.reshape(-1)).double().norm() / r.double().norm()).item()
           for k, g, r in zip(names, got, ref)}
    res["against_torch"] = {"shape": f"{a.torch_ng} Gaussians x 64^3, cutoff {CUTOFF}", "hip_voxelize_backward": hip_b,
                            "hip_voxelize": hip_f, "torch_autograd_forward_plus_backward": tor,
                            "speedup_backward_alone": tor["median_ms"] / hip_b["median_ms"],
                            "speedup_forward_plus_backward": tor["median_ms"] / (hip_b["median_ms"] + hip_f["median_ms"]),
                            "rel_l2_hip_vs_torch_fp32": rel}
    print("torch", res["against_torch"], flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": "voxelize_backward: torch autograd (fwd+bwd) / HIP backward, 2000 x 64^3",
                      "value": res["against_torch"]["speedup_backward_alone"]}))


if __name__ == "__main__":
    main()
