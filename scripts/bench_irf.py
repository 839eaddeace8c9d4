"""Temporal-response timing at the C3 volume (128 x 128 wall points x 1024 bins) for IRFs of 1, 33, 129 and
512 taps: (a) nlosgr_mse, the loss of an ideal detector; (b) nlosgr_mse_irf, the fused loss through the IRF;
(c) the same loss and gradient composed from torch ops (conv1d, MSE, autograd.grad), what a user would write
without (b); (d) nlosgr_loss_irf with the Poisson deviance of photon counts in place of the MSE (rate_floor 1).
Warm-up, timed repeats, device-event timing, one process; writes one JSON file and prints the
markdown table of DESIGN §7.  (b) - (a) is also given as a share of the C3 training step
(profiles/r06_c3_bench.json).

    python scripts/bench_irf.py [--out profiles/irf_c3.json] [--rows 16384] [--nr 1024] [--repeats 9]
    python scripts/bench_irf.py --out profiles/loss_poisson_c3.json     # the record of column (d)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nlosgr.irf import IRF  # noqa: E402
from nlosgr.loss import loss as fused_loss  # noqa: E402
from nlosgr.train import mse  # noqa: E402

DEV = torch.device("cuda:0")
TAPS = (1, 33, 129, 512)
GT = 100.0


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


def make_irf(L):
    """L taps: the identity at L = 1, else a Gaussian peak at L / 3 with an exponential tail, normalised."""
    if L == 1:
        return IRF([1.0], 0, 0.0)
    k = torch.arange(L, dtype=torch.float64) - L // 3
    w = torch.exp(-0.5 * (k / (L / 14.0)) ** 2) + 0.3 * torch.exp(-k.clamp_min(0) / (L / 8.0)) * (k > 0)
    return IRF(w / w.sum(), L // 3, 1e-3)


def torch_route(hist, target, irf):
    """(loss, dL/dhist) from torch ops: conv1d correlates, so flipped taps and pad (L-1-c, c)."""
    L, c = len(irf), irf.center
    kern = irf.taps.flip(0).view(1, 1, L)
    h = hist.detach().requires_grad_(True)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(h.unsqueeze(1), (L - 1 - c, c)), kern).squeeze(1)
    loss = ((y + irf.background - target * GT) ** 2).mean()
    (g,) = torch.autograd.grad(loss, h)
    return loss, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irf_c3.json"))
    ap.add_argument("--rows", type=int, default=128 * 128)
    ap.add_argument("--nr", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_irf needs a GPU"
    g = torch.Generator().manual_seed(0)
    hist = torch.rand(a.rows, a.nr, generator=g).to(DEV)
    target = (torch.rand(a.rows, a.nr, generator=g) * 1e-2).to(DEV)
    step_ms = None
    try:
        with open(os.path.join(ROOT, "profiles", "r06_c3_bench.json")) as fh:
            step_ms = json.load(fh)["ms_per_step"]
    except (OSError, KeyError, ValueError):
        pass
    res = {"workload": f"hist, target [{a.rows}, {a.nr}] fp32 (hist ~ U(0,1), target ~ 1e-2 U, gt_times {GT})",
           "device": torch.cuda.get_device_name(0), "timing": "device events around each call, median of repeats",
           "c3_step_ms": step_ms, "taps": {}}
    base = stats(timed(lambda: mse(hist, target, GT, raw=True), a.warmup, a.repeats))
    res["nlosgr_mse"] = base
    print("nlosgr_mse", base, flush=True)
    for L in TAPS:
        irf = make_irf(L).to(DEV)
        e = {"center": irf.center}
        e["nlosgr_mse_irf"] = stats(timed(lambda: mse(hist, target, GT, raw=True, irf=irf), a.warmup, a.repeats))
        e["nlosgr_loss_irf_poisson"] = stats(timed(lambda: fused_loss(hist, target, GT, raw=True, irf=irf, kind="poisson",
                                                                      rate_floor=1.0), a.warmup, a.repeats))
        e["poisson_extra_ms_over_mse_irf"] = e["nlosgr_loss_irf_poisson"]["median_ms"] - e["nlosgr_mse_irf"]["median_ms"]
        try:
            e["torch_conv1d_mse_autograd"] = stats(timed(lambda: torch_route(hist, target, irf), a.warmup, a.repeats))
            loss4, grad = mse(hist, target, GT, raw=True, irf=irf)
            tl, tg = torch_route(hist, target, irf)
            e["rel_vs_torch"] = {"loss": abs(loss4[0].item() - tl.item()) / tl.item(),
                                 "grad_l2": ((grad - tg).double().norm() / tg.double().norm()).item()}
            e["speedup_vs_torch"] = e["torch_conv1d_mse_autograd"]["median_ms"] / e["nlosgr_mse_irf"]["median_ms"]
        except RuntimeError as err:   # (e.g. out of memory in the torch route)
            e["torch_conv1d_mse_autograd"] = {"error": str(err).splitlines()[0][:200]}
            torch.cuda.empty_cache()
        e["extra_ms_over_mse"] = e["nlosgr_mse_irf"]["median_ms"] - base["median_ms"]
        if step_ms:
            e["extra_share_of_c3_step"] = e["extra_ms_over_mse"] / step_ms
        res["taps"][str(L)] = e
        print(L, e, flush=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("| taps | nlosgr_mse (ms) | nlosgr_mse_irf (ms) | torch conv1d + MSE + autograd (ms) | (b) - (a) of the C3 step "
          "| nlosgr_loss_irf POISSON (ms) |")
    print("|---|---|---|---|---|---|")
    for L in TAPS:
        e = res["taps"][str(L)]
        t = e["torch_conv1d_mse_autograd"]
        tt = f"{t['median_ms']:.2f}" if "median_ms" in t else "failed"
        sh = f"{100 * e['extra_share_of_c3_step']:.3f} %" if step_ms else "n/a"
        print(f"| {L} | {base['median_ms']:.3f} | {e['nlosgr_mse_irf']['median_ms']:.3f} | {tt} | {sh} "
              f"| {e['nlosgr_loss_irf_poisson']['median_ms']:.3f} |")
    worst = min((e.get("speedup_vs_torch", float("inf")) for e in res["taps"].values()))
    print(json.dumps({"metric": "nlosgr_mse_irf vs torch composition, worst speedup over the tap counts", "value": worst}))


if __name__ == "__main__":
    main()
