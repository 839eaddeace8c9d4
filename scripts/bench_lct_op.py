"""LCT operator pair timing at 128 x 128 wall points x 1024 bins, nv = 1024 (work arrays 256 x 256 x 2048 complex64,
1 GiB): each of the four new passes (load_volume, store_rows, load_rows, store_volume) against its minimum traffic
computed from the shapes, LctOperator.forward and .adjoint, and one lct_solve iteration, against
  - lct_reconstruct(inverse=) in the same process, the yardstick: the same two FFTs and passes of the same traffic,
  - forward_project and backproject on the same walls and the operator's own voxels (fk_grid), the exact pair the
    operator replaces, and
  - A as a torch composition: dense R matmuls on both sides, pad, fftn, a product with Fk, ifftn, the weight.
bench_lct.py's method: the variants alternate in one process, the median of the rounds after the warm-ups with min
and max; a stage is --inner back-to-back calls between two device events, a whole call one call.  Writes one JSON file.

    python scripts/bench_lct_op.py [--out profiles/lct_op_c3.json] [--repeats 10] [--wall 128] [--nr 1024] [--nv 1024]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_fk import stats, timed_alternating  # noqa: E402
from nlosgr import lct as LCT  # noqa: E402
from nlosgr.backproject import backproject  # noqa: E402
from nlosgr.forward_project import forward_project  # noqa: E402

DEV = torch.device("cuda:0")


class TorchForward:
    """A of include/nlosgr.h as torch calls; R (dense, fp32), the weights and Fk are built once."""

    def __init__(self, op):
        self.H, self.W, self.nv = op.H, op.W, op.nv
        self.R = op.resampling.dense().float().to(DEV)                           # [nv, nr]
        self.Rt = self.R.t().contiguous()
        r = op.r0 + op.dr * torch.arange(op.nr, dtype=torch.float64)
        self.w = (r ** op.power).float().to(DEV)
        self.Fk = op.Fk

    def __call__(self, volume):
        H, W, nv = self.H, self.W, self.nv
        pad = torch.zeros(2 * H, 2 * W, 2 * nv, device=DEV)
        pad[:H, :W, :nv] = volume.permute(2, 0, 1) @ self.Rt
        o = torch.fft.ifftn(torch.fft.fftn(pad) * self.Fk)
        return ((o[:H, :W, :nv].real @ self.R) * self.w).reshape(H * W, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lct_op_c3.json"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls between the events of a stage timing")
    ap.add_argument("--wall", type=int, default=128)
    ap.add_argument("--nr", type=int, default=1024)
    ap.add_argument("--nv", type=int, default=None, help="depth-squared cells (default: nr)")
    ap.add_argument("--exact-repeats", type=int, default=3, help="rounds of the exact projector pair (it is slow)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lct_op needs a GPU"
    H = W = a.wall
    nr = a.nr
    dr = 1.28 / 1024
    I1 = nr // 8
    r0 = I1 * dr
    sx = sz = 1.0 / a.wall
    g = torch.Generator().manual_seed(0)
    rows = torch.rand(H * W, nr, generator=g).to(DEV)
    volume = torch.rand(W, nr, H, generator=g).to(DEV)

    op = LCT.LctOperator(H, W, sx, sz, r0, dr, nr, power=0, nv=a.nv, device=DEV)
    res, nv = op.resampling, op.nv
    pad = torch.empty((2 * H, 2 * W, 2 * nv), dtype=torch.complex64, device=DEV)
    field = torch.fft.ifftn(torch.fft.fftn(LCT.lct_load_volume(volume, res, out=pad)))
    rows_out = torch.empty_like(rows)
    stages = {
        "load_volume": lambda: LCT.lct_load_volume(volume, res, out=pad),
        "store_rows": lambda: LCT.lct_store_rows(field, res, out=rows_out),
        "load_rows": lambda: LCT.lct_load_rows(rows, H, W, r0, dr, resampling=res, out=pad),
        "store_volume": lambda: LCT.lct_store_volume(field, res),
        "load": lambda: LCT.lct_load(rows, H, W, r0, dr, resampling=res, out=pad),
        "store": lambda: LCT.lct_store(field, res),
    }
    ms = timed_alternating(stages, a.warmup, a.repeats, inner=a.inner)
    A = 8 * (2 * H) * (2 * W) * (2 * nv)                    # bytes of a work array
    small = 4 * H * W * nr                                  # the rows, or the volume
    traffic = {"load_volume": small + A, "load_rows": small + A, "load": small + A,   # read once, the array written once
               "store_rows": A // 8 + small, "store_volume": A // 8 + small, "store": A // 8 + small}  # the corner read
    out = {"workload": f"{H} x {W} wall (spacing 1 / {a.wall}), {nr} bins of c deltaT = 1.28 / 1024 from bin {I1}, "
                       f"nv = {nv} cells, power 0, uniform-random rows and volume (seed 0); work arrays {2 * H} x "
                       f"{2 * W} x {2 * nv} complex64 ({A / 2 ** 30:.3g} GiB); resampling tables of {res.nnz} weights",
           "device": torch.cuda.get_device_name(0),
           "timing": f"variants alternating in one process, median of the rounds; stages: device events around {a.inner} "
                     "back-to-back calls, time per call; totals: device events around one call",
           "stages": {k: stats(v) for k, v in ms.items()}, "min_traffic_bytes": traffic}
    for k, nbytes in traffic.items():
        out["stages"][k]["achieved_TB_per_s"] = nbytes / (out["stages"][k]["median_ms"] * 1e-3) / 1e12
    del pad, field

    G = LCT.lct_inverse(H, W, nv, sx, sz, res.dv, 0.8, device=DEV)
    tf = TorchForward(op)
    step = 1.0 / op.norm()
    totals = timed_alternating({
        "forward": lambda: op.forward(volume),
        "adjoint": lambda: op.adjoint(rows),
        "lct_solve_one_iteration": lambda: LCT.lct_solve(rows, op, iterations=1, step=step, x0=volume),
        "lct_solve_one_fista_iteration": lambda: LCT.lct_solve(rows, op, iterations=1, step=step, x0=volume,
                                                               accelerate=True),
        "lct_reconstruct_inverse_given": lambda: LCT.lct_reconstruct(rows, H, W, sx, sz, r0, dr, nv=a.nv, inverse=G),
        "torch_composition_forward": lambda: tf(volume),
    }, a.warmup, a.repeats)
    out["totals"] = {k: stats(v) for k, v in totals.items()}
    got, want = op.forward(volume), tf(volume)
    out["forward_max_diff_vs_torch_composition_of_max"] = float((got - want).abs().max() / want.abs().max())
    out["bitwise_repeatable"] = bool(torch.equal(got, op.forward(volume))
                                     and torch.equal(op.adjoint(rows), op.adjoint(rows)))
    v64, h64 = volume.double(), rows.double()
    Av, Ath = got.double(), op.adjoint(rows).double()
    out["adjoint_identity_gap"] = float(((Av * h64).sum() - (v64 * Ath).sum()).abs() / (Av.norm() * h64.norm()))
    del G, tf, got, want, v64, h64, Av, Ath

    # the exact pair on the same walls and voxels: every (voxel, wall point) pair
    xs = ((np.arange(W) - (W - 1) / 2) * sx).astype(np.float32)
    zs = ((np.arange(H) - (H - 1) / 2) * sz).astype(np.float32)
    zz, xx = np.meshgrid(zs, xs, indexing="ij")
    walls = torch.from_numpy(np.stack([xx.reshape(-1), np.zeros(H * W, dtype=np.float32), zz.reshape(-1)], axis=1)).to(DEV)
    grid = op.grid(xs, zs, 0.0)
    exact = timed_alternating({
        "forward_project": lambda: forward_project(volume, walls, grid, r0, dr, nr, power=0),
        "backproject": lambda: backproject(rows, walls, grid, r0, dr, power=0),
    }, 1, a.exact_repeats)
    out["totals"].update({k: stats(v) for k, v in exact.items()})

    t = {k: v["median_ms"] for k, v in out["totals"].items()}
    yard = t["lct_reconstruct_inverse_given"]
    out["ratios"] = {"forward_over_lct_reconstruct": t["forward"] / yard, "adjoint_over_lct_reconstruct": t["adjoint"] / yard,
                     "forward_over_torch_composition": t["forward"] / t["torch_composition_forward"],
                     "forward_project_over_forward": t["forward_project"] / t["forward"],
                     "backproject_over_adjoint": t["backproject"] / t["adjoint"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))
    print(json.dumps({"metric": f"LCT operator {H} x {W} x {nr}: forward ms", "value": t["forward"]}))


if __name__ == "__main__":
    main()
