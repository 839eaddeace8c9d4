"""Primal-dual LCT iteration timing at 128 x 128 wall points x 1024 bins, nv = 1024: each of the three new passes
(nlosgr_prox_rows for both data terms, nlosgr_tv_dual, nlosgr_tv_primal) against its minimum traffic computed from the
shapes and against the same update composed from torch calls, and one whole iteration of lct_solve_pd against
  - the same iteration with the three passes as torch calls on the same LctOperator, and
  - one lct_solve iteration (the two operator applications and torch's residual, step and clamp).
bench_lct.py's method: the variants alternate in one process, the median of the rounds after the warm-ups with min
and max; a pass is --inner back-to-back calls between two device events, a whole iteration one call.  Writes one JSON
file.

    python scripts/bench_lct_pd.py [--out profiles/lct_pd_c3.json] [--repeats 10] [--wall 128] [--nr 1024] [--nv 1024]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

from bench_fk import stats, timed_alternating  # noqa: E402
from nlosgr import lct as LCT  # noqa: E402
from nlosgr import prox as PX  # noqa: E402

DEV = torch.device("cuda:0")


def torch_rows_mse(q, z, h, sigma):
    F = 0.5 * (z - h).double().square().sum()
    q.add_(z, alpha=sigma).sub_(h, alpha=sigma).div_(1.0 + sigma)
    return F


def torch_rows_poisson(q, z, h, e, sigma, gt, eps):
    yp = (gt * h).clamp_min(0.0) + eps
    rho = ((e[None] * z).clamp_min(0.0) + eps).double()
    t = (rho - yp.double()) / yp.double()
    F = (yp.double() * (t - torch.log1p(t))).sum()
    d = e[None]
    sp = sigma / (d * d)
    s = (q + sigma * z) / d + sp * eps
    D = torch.sqrt((s - 1.0) ** 2 + 4.0 * sp * yp)
    q.copy_(torch.where(d > 0, d * 2.0 * (s - sp * yp) / (1.0 + s + D), torch.zeros_like(q)))
    return F


def torch_gradient(x, a):
    g = torch.zeros((3,) + tuple(x.shape), device=x.device)
    g[0, :-1] = a[0] * (x[1:] - x[:-1])
    g[1, :, :-1] = a[1] * (x[:, 1:] - x[:, :-1])
    g[2, :, :, :-1] = a[2] * (x[:, :, 1:] - x[:, :, :-1])
    return g


def torch_dual(p, xbar, sigma, tv, a):
    g = torch_gradient(xbar, a)
    sums = torch.stack([g.double().square().sum(dim=0).sqrt().sum(), xbar.double().abs().sum()])
    p.add_(g, alpha=sigma)
    n = p.square().sum(dim=0).sqrt()
    p.mul_(torch.clamp(tv / n, max=1.0)[None])
    return sums


def torch_primal(x, xbar, g, p, tau, l1, a):
    d = g.clone()
    d[1:] += a[0] * p[0, :-1]
    d[:-1] -= a[0] * p[0, :-1]
    d[:, 1:] += a[1] * p[1, :, :-1]
    d[:, :-1] -= a[1] * p[1, :, :-1]
    d[:, :, 1:] += a[2] * p[2, :, :, :-1]
    d[:, :, :-1] -= a[2] * p[2, :, :, :-1]
    xp = (x - tau * d - tau * l1).clamp_min_(0.0)
    torch.sub(2.0 * xp, x, out=xbar)
    x.copy_(xp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lct_pd_c3.json"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls between the events of a pass timing")
    ap.add_argument("--wall", type=int, default=128)
    ap.add_argument("--nr", type=int, default=1024)
    ap.add_argument("--nv", type=int, default=None, help="depth-squared cells (default: nr)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lct_pd needs a GPU"
    H = W = a.wall
    nr = a.nr
    dr = 1.28 / 1024
    I1 = nr // 8
    r0 = I1 * dr
    sx = sz = 1.0 / a.wall
    g = torch.Generator().manual_seed(0)
    rows = (torch.rand(H * W, nr, generator=g) * 20.0).to(DEV)
    volume = torch.rand(W, nr, H, generator=g).to(DEV)
    weights = (1.0, 1.0, 1.0)
    sigma = tau = 0.05
    tv, l1, gt, eps = 0.3, 0.01, 1.0, 1.0
    exposure = (r0 + dr * torch.arange(nr, dtype=torch.float64)).pow(-3.0).float().to(DEV)

    # ---- the three passes alone, against their torch compositions ----------------------------------------------
    z = (torch.rand(H * W, nr, generator=g) * 20.0).to(DEV)
    q = torch.randn(H * W, nr, generator=g).to(DEV)
    q2 = q.clone()
    x, xbar, grad = volume.clone(), torch.rand(W, nr, H, generator=g).to(DEV), torch.randn(W, nr, H, generator=g).to(DEV)
    p = torch.randn(3, W, nr, H, generator=g).to(DEV)
    x2, xbar2, p2 = x.clone(), xbar.clone(), p.clone()
    # the updates run in place on their own arrays: the values drift over the repeats, the traffic does not
    passes = {
        "prox_rows_mse": lambda: PX.prox_rows(q, z, rows, H, W, sigma),
        "prox_rows_poisson": lambda: PX.prox_rows(q, z, rows, H, W, sigma, "poisson", exposure, gt, eps),
        "tv_dual": lambda: PX.tv_dual_step(p, xbar, sigma, tv, weights),
        "tv_primal": lambda: PX.tv_primal_step(x, xbar, grad, p, tau, l1, weights),
        "torch_rows_mse": lambda: torch_rows_mse(q2, z, rows, sigma),
        "torch_rows_poisson": lambda: torch_rows_poisson(q2, z, rows, exposure, sigma, gt, eps),
        "torch_dual": lambda: torch_dual(p2, xbar2, sigma, tv, weights),
        "torch_primal": lambda: torch_primal(x2, xbar2, grad, p2, tau, l1, weights),
    }
    ms = timed_alternating(passes, a.warmup, a.repeats, inner=a.inner)
    nvox, nrow = W * nr * H, H * W * nr
    traffic = {"prox_rows_mse": 4 * 4 * nrow, "prox_rows_poisson": 4 * 4 * nrow,     # z, h, q read; q written
               "tv_dual": 7 * 4 * nvox,                                               # xbar, p read; p written
               "tv_primal": 7 * 4 * nvox}                                             # p, g, x read; x, xbar written
    out = {"workload": f"{H} x {W} wall, {nr} bins from bin {I1}, volume {W} x {nr} x {H}; uniform-random rows, volume "
                       f"and duals (seed 0); sigma = tau = {sigma}, tv {tv}, l1 {l1}, unit axis weights, the exposure "
                       "r^-3",
           "device": torch.cuda.get_device_name(0),
           "timing": f"variants alternating in one process, median of the rounds; passes: device events around {a.inner} "
                     "back-to-back calls, time per call; iterations: device events around one call",
           "passes": {k: stats(v) for k, v in ms.items()}, "min_traffic_bytes": traffic}
    for k, nbytes in traffic.items():
        out["passes"][k]["achieved_GB_per_s"] = nbytes / (out["passes"][k]["median_ms"] * 1e-3) / 1e9
    med = lambda k: out["passes"][k]["median_ms"]
    hip3 = med("prox_rows_mse") + med("tv_dual") + med("tv_primal")
    torch3 = med("torch_rows_mse") + med("torch_dual") + med("torch_primal")
    out["three_passes_ms"] = {"hip_mse": hip3, "torch_mse": torch3,
                              "hip_poisson": hip3 - med("prox_rows_mse") + med("prox_rows_poisson"),
                              "torch_poisson": torch3 - med("torch_rows_mse") + med("torch_rows_poisson")}
    del q2, x2, xbar2, p2, grad

    # ---- one whole iteration -------------------------------------------------------------------------------------
    op = LCT.LctOperator(H, W, sx, sz, r0, dr, nr, power=0, nv=a.nv, device=DEV)
    norm = LCT.NORM_SAFETY * op.norm()
    step = PX.default_steps(norm, tv, weights)
    zbuf = torch.empty_like(rows)

    def hip_iteration(loss="mse", e=None):
        op.forward(xbar, out=zbuf)
        PX.prox_rows(q, zbuf, rows, H, W, step, loss, e, gt, eps)
        PX.tv_dual_step(p, xbar, step, tv, weights)
        PX.tv_primal_step(x, xbar, op.adjoint(q), p, step, l1, weights)

    def torch_iteration():
        op.forward(xbar, out=zbuf)
        torch_rows_mse(q, zbuf, rows, step)
        torch_dual(p, xbar, step, tv, weights)
        torch_primal(x, xbar, op.adjoint(q), p, step, l1, weights)

    totals = timed_alternating({
        "primal_dual_iteration": hip_iteration,
        "primal_dual_iteration_poisson": lambda: hip_iteration("poisson", exposure),
        "torch_composition_iteration": torch_iteration,
        "lct_solve_one_iteration": lambda: LCT.lct_solve(rows, op, iterations=1, step=1.0 / norm, x0=volume),
        "lct_solve_pd_one_iteration": lambda: LCT.lct_solve_pd(rows, op, iterations=1, tv=tv, l1=l1, norm=norm, x0=volume),
    }, a.warmup, a.repeats)
    out["iterations"] = {k: stats(v) for k, v in totals.items()}
    it = lambda k: out["iterations"][k]["median_ms"]
    out["ratios"] = {"three_passes_hip_over_torch_mse": hip3 / torch3,
                     "three_passes_hip_over_torch_poisson": out["three_passes_ms"]["hip_poisson"]
                                                            / out["three_passes_ms"]["torch_poisson"],
                     "iteration_hip_over_torch_composition": it("primal_dual_iteration") / it("torch_composition_iteration"),
                     "iteration_over_lct_solve_iteration": it("primal_dual_iteration") / it("lct_solve_one_iteration")}
    # the torch composition computes what the passes compute
    torch.manual_seed(1)
    xa, pa = torch.rand(W, nr, H, device=DEV), torch.randn(3, W, nr, H, device=DEV)
    pb = pa.clone()
    sa, sb = PX.tv_dual_step(pa, xa, sigma, tv, weights), torch_dual(pb, xa, sigma, tv, weights)
    out["dual_max_diff_vs_torch"] = float((pa - pb).abs().max())
    out["dual_sums_rel_diff_vs_torch"] = float(((sa - sb).abs() / sb).max())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"passes_ms": {k: round(v["median_ms"], 4) for k, v in out["passes"].items()},
                      "GB_per_s": {k: round(out["passes"][k]["achieved_GB_per_s"], 1) for k in traffic},
                      "iterations_ms": {k: round(v["median_ms"], 3) for k, v in out["iterations"].items()},
                      "ratios": out["ratios"]}))


if __name__ == "__main__":
    main()
