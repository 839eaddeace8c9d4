"""The non-confocal Gaussian renderer against the confocal pair-major one, timed in the same process on a C3-like
scene: 100k synthetic Gaussians (bench.py's), 32 x 32 rays, 1024 bins of c deltaT = 1.28 / 1024 from bin 128, 5.7
sigma, and as the wall a 1024-measurement row-interleaved shard of the 128 x 128 wall (rows 0, 16, ...:
distributed.wall_rows), so that a run stays short.  Four forward / backward pairs:

    confocal      render_forward / render_backward (the pair-major FX drain and backward, unchanged)
    same          render_nc_forward / render_nc_backward with lasers == sensors
    displaced     the same with every laser displaced by up to +-0.1 in x and z
    one_laser     the same with one spot for the shard

The variants are timed alternating (one call of each per round), device events around each call, median of
--repeats rounds after --warmup untimed rounds.  Also records nlosgr_count_support's (pairs, rays, evaluations) of
the confocal case.  Writes one JSON file and prints the ratios to the confocal times.

    python scripts/bench_render_nc.py [--out profiles/render_nc_c3.json] [--repeats 5] [--warmup 1] [--gaussians N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

H = W = 128
T, NS, SHARDS, CUTOFF = 1024, 32, 16, 5.7


def alternating(fns, warmup, repeats):
    """{name: [ms]}: `repeats` rounds of one call of each function, device events around each call."""
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


def stats(ms, base=None):
    s = sorted(ms)
    d = {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "repeats": len(s)}
    if base:
        d["ratio_to_confocal"] = d["median_ms"] / base
    return d


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_nc_c3.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gaussians", type=int, default=100_000)
    a = ap.parse_args(argv)
    from nlosgr import GaussianParams, features_flat
    from nlosgr.distributed import wall_rows
    from nlosgr.render import count_support, render_backward, render_forward
    from nlosgr.render_nc import render_nc_backward, render_nc_forward
    from nlosgr.volume import Scene, make_config
    dev = torch.device("cuda:0")
    scene = Scene(H=H, W=W, T=T, ns=NS)
    model = GaussianParams.synthetic(a.gaussians, 3, preset="cuda", device=dev, seed=0)
    idx = wall_rows(H, W, 0, SHARDS, device=dev)
    geo = scene.geometry(dev, "cuda", "noocl", walls=scene.walls(dev)[idx].contiguous())
    cfg = make_config(model, scene, "cuda", "noocl", cutoff=CUTOFF)
    args = [model._mu.detach(), model._scaling.detach(), model._rotation.detach(), model._opacity.detach(),
            features_flat(model).detach().contiguous()]
    g = torch.Generator().manual_seed(1)
    grad = torch.randn(geo.nwall, geo.nr, generator=g).to(dev)
    d = (torch.rand(geo.nwall, 3, generator=g) * 2 - 1) * 0.1
    d[:, 1] = 0.0
    lasers = {"same": geo.wall.clone(), "displaced": (geo.wall + d.to(dev)).contiguous(),
              "one_laser": torch.tensor([[0.1, 0.0, -0.05]], device=dev)}
    fwd = {"confocal": lambda: render_forward(*args, geo, cfg)}
    bwd = {"confocal": lambda: render_backward(*args, geo, cfg, grad_hist=grad)}
    for k, l in lasers.items():
        fwd[k] = (lambda l=l: render_nc_forward(*args, geo, l, cfg))
        bwd[k] = (lambda l=l: render_nc_backward(*args, geo, l, cfg, grad))
    tf, tb = alternating(fwd, a.warmup, a.repeats), alternating(bwd, a.warmup, a.repeats)
    bf, bb = stats(tf["confocal"])["median_ms"], stats(tb["confocal"])["median_ms"]
    pairs, rays, evals = count_support(*args, geo, cfg)
    same = render_nc_forward(*args, geo, lasers["same"], cfg)
    conf = render_forward(*args, geo, cfg)[0]
    from dataclasses import replace
    from nlosgr import _lib
    flt = render_forward(*args, geo, replace(cfg, flags=_lib.FLAG_FLOAT_DRAIN))[0]   # the fp32 claim drain
    rel = lambda x, y: float(((x - y).abs().amax(1) / y.abs().amax(1)).max())
    res = {
        "workload": f"{a.gaussians} synthetic Gaussians (seed 0, cuda preset), {geo.nwall} measurements (rows 0, "
                    f"{SHARDS}, ... of a {H} x {W} wall), {NS} x {NS} rays, {T} bins of 1.28 / {T} from bin {T // 8}, "
                    f"cutoff {CUTOFF}",
        "device": torch.cuda.get_device_name(dev),
        "timing": "the variants alternating, device events around each call, median of the rounds",
        "confocal_support": {"pairs": pairs, "rays": rays, "evaluations": evals},
        "max_difference_of_rowmax": {"same_vs_confocal_fx_drain": rel(same, conf), "same_vs_confocal_float_drain":
                                     rel(same, flt), "confocal_fx_vs_float_drain": rel(conf, flt)},
        "forward": {k: stats(v, bf) for k, v in tf.items()},
        "backward": {k: stats(v, bb) for k, v in tb.items()},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for phase in ("forward", "backward"):
        print(phase + ": " + ", ".join(f"{k} {v['median_ms']:.1f} ms (x{v['ratio_to_confocal']:.1f})"
                                       for k, v in res[phase].items()))
    print("max difference / rowmax: " + ", ".join(f"{k} {v:.2e}" for k, v in res["max_difference_of_rowmax"].items()))
    print(f"confocal support: {pairs} pairs, {rays} rays, {evals} evaluations; wrote {a.out}")


if __name__ == "__main__":
    main()
