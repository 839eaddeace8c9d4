"""SGLD noise timing: nlosgr_sgld_noise (one launch, one thread per Gaussian) beside nlosgr_adam on the same model
(the launch it follows in a train step) and beside the composition available without it in torch: randn, the gate,
the covariance from quaternion and scales, bmm, add.  Models of 1e5 (C3's size) and 1e6 synthetic cuda-preset
Gaussians of SH degree 3.  The three variants alternate in one process, device events around each call, the median
after a warm-up.  --c3-step also times the flagship training step (bench.py's C3: 1e5 Gaussians, a 128 x 128 wall,
1024 bins, cutoff 5.7) with noise_lr = 0 and 5e5, alternating, the model and the Adam state put back after every step.
Writes one JSON file.  No gate: nothing is tuned to these numbers.

    python scripts/bench_sgld.py [--out profiles/sgld.json] [--repeats 5] [--c3-step]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nlosgr import GaussianParams  # noqa: E402
from nlosgr.train import Adam, OptimizationParams, sgld_noise  # noqa: E402

DEV = torch.device("cuda:0")
LR_MU, NOISE_LR, GATE_K, GATE_X0 = 1.6e-4, 5e5, 100.0, 0.995


def timed_alternating(fns, warmup, repeats):
    """{name: [ms]}: the variants run in turn, `repeats` rounds, device events around each call."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "repeats": len(s)}


def torch_noise(m, scale):
    """The same update from torch operators (cuda preset, torch.randn in place of the counter-based generator)."""
    with torch.no_grad():
        xi = torch.randn_like(m._mu)
        sig = torch.sigmoid(m._opacity.reshape(-1))
        gate = torch.sigmoid(GATE_K * ((1.0 - sig) - GATE_X0))
        s2 = (torch.exp(m._scaling) + 1e-8).square()
        q = torch.nn.functional.normalize(m._rotation)
        w, x, y, z = q.unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
        cov = torch.bmm(R * s2[:, None, :], R.transpose(1, 2))
        m._mu.data.add_((scale * gate)[:, None] * torch.bmm(cov, xi[:, :, None]).squeeze(-1))


def c3_step(warmup, repeats):
    """The C3 step with and without the noise: {"plain": stats, "noise": stats} (whole steps, device events)."""
    from nlosgr.train import TrainStep
    from nlosgr.volume import Scene, make_config
    ng, H, W, T, ns = 100_000, 128, 128, 1024, 32
    scene = Scene(H=H, W=W, T=T, ns=ns)
    model = GaussianParams.synthetic(ng, 3, preset="cuda", device=DEV, seed=0)
    model._opacity.data[::10] = -8.0                  # a tenth nearly transparent: the gate lets them move
    cfg = make_config(model, scene, "cuda", "noocl", cutoff=5.7)
    geo = scene.geometry(DEV, "cuda", "noocl")
    target = (torch.rand(H * W, T, generator=torch.Generator().manual_seed(1)) * 1e-3).to(DEV)
    steps = {"plain": TrainStep(model, geo, cfg, target, gt_times=100.0),
             "noise": TrainStep(model, geo, cfg, target, gt_times=100.0,
                                opt=OptimizationParams(noise_lr=NOISE_LR))}
    saved = [t.clone() for t in steps["plain"]._tensors]

    def restore(step):
        """The frozen workload again (outside the events): parameters, Adam moments and counters."""
        for t, s0 in zip(step._tensors, saved):
            t.copy_(s0)
        for m1, m2 in zip(step.adam.exp_avg, step.adam.exp_avg_sq):
            m1.zero_()
            m2.zero_()
        step.adam.step_count = step.iteration = 0

    def timed(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        restore(step)
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        for st in steps.values():
            timed(st)
    ms = {k: [] for k in steps}
    for _ in range(repeats):
        for k, st in steps.items():
            ms[k].append(timed(st))
    out = {k: stats(v) for k, v in ms.items()}
    out["noise_minus_plain_ms"] = out["noise"]["median_ms"] - out["plain"]["median_ms"]
    out["workload"] = f"C3: {ng} Gaussians, {H} x {W} wall, {T} bins, {ns} x {ns} rays, cuda preset, cutoff 5.7"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgld.json"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--c3-step", action="store_true", help="also time the C3 training step with and without noise")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sgld needs a GPU"
    res = {"workload": "synthetic cuda-preset Gaussians of SH degree 3, a tenth of them nearly transparent (raw opacity "
                       f"-8); noise_lr {NOISE_LR:g} x lr_mu {LR_MU:g}, gate {GATE_K:g} / {GATE_X0}",
           "device": torch.cuda.get_device_name(0),
           "timing": "sgld, adam and torch alternating in one process, device events around each call, median of the "
                     "rounds after the warm-up",
           "sgld": "train.sgld_noise (nlosgr_sgld_noise, in place on _mu)",
           "adam": "train.Adam.step over the six parameter groups of the same model (nlosgr_adam)",
           "torch": "randn + sigmoid gate + quaternion -> R, R diag(s^2) R^T, bmm, add_", "cases": {}}
    for ng in (100_000, 1_000_000):
        m = GaussianParams.synthetic(ng, 3, preset="cuda", device=DEV, seed=0)
        m._opacity.data[::10] = -8.0
        tensors = [m._mu.data, m._features_dc.data.view(ng, -1), m._features_rest.data.view(ng, -1),
                   m._opacity.data.view(ng), m._scaling.data, m._rotation.data]
        adam = Adam(tensors)
        grads = [1e-3 * torch.randn_like(t) for t in tensors]
        o = OptimizationParams()
        lrs = [LR_MU, o.feature_lr, o.feature_lr / 20.0, o.opacity_lr, o.scaling_lr, o.rotation_lr]
        it = [0]

        def sgld():
            sgld_noise(m, LR_MU, NOISE_LR, it[0], seed=0, preset="cuda", gate_k=GATE_K, gate_x0=GATE_X0)
            it[0] += 1

        ms = timed_alternating({"sgld": sgld, "adam": lambda: adam.step(grads, lrs),
                                "torch": lambda: torch_noise(m, NOISE_LR * LR_MU)}, a.warmup, a.repeats)
        e = {k: stats(v) for k, v in ms.items()}
        e["bytes_sgld"] = ng * 14 * 4
        e["gb_per_s_sgld"] = e["bytes_sgld"] / (e["sgld"]["median_ms"] * 1e-3) / 1e9
        e["sgld_over_adam"] = e["sgld"]["median_ms"] / e["adam"]["median_ms"]
        e["sgld_over_torch"] = e["sgld"]["median_ms"] / e["torch"]["median_ms"]
        res["cases"][str(ng)] = e
        print(ng, e, flush=True)
    if a.c3_step:
        res["c3_step"] = c3_step(a.warmup, 3)
        print("c3_step", res["c3_step"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": "nlosgr_sgld_noise at 1e5 Gaussians, median ms",
                      "value": res["cases"]["100000"]["sgld"]["median_ms"]}))


if __name__ == "__main__":
    main()
