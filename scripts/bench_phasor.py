"""Phasor-field gather timing: nlosgr_backproject_phasor (one pass over interleaved complex rows) against the
composition available without it: two real back-projections (one per channel) plus torch.hypot.  The workload is
scripts/bench_backproject.py's: a 256 x 256 wall with C3's window (1024 bins of c deltaT = 1.28 / 1024 from bin
128) onto 128^3 voxels, for a confocal capture, one laser spot per measurement and one spot for the capture.  The
rows are uniform-random rows filtered with the Morlet wavelet (phasor_rows), so both routes read the same numbers.
The two variants alternate in one process, device events around each call, the median after a warm-up; the planes
of the two routes are compared bitwise at the timed size.  The time filter is timed beside them.  Writes one JSON
file.  NLOSGR_LIB selects an alternative in-tree build (A/B of the kernel's group size); --label names it.

    python scripts/bench_phasor.py [--out profiles/phasor_bp.json] [--repeats 5] [--power 0] [--res 128]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nlosgr.backproject import backproject  # noqa: E402
from nlosgr.geometry import relay_wall_grid  # noqa: E402
from nlosgr.phasor import phasor_backproject, phasor_kernel, phasor_rows  # noqa: E402
from nlosgr.voxelize import VoxelGrid  # noqa: E402

DEV = torch.device("cuda:0")
POS, SIZE = (0.0, 0.5, 0.0), 0.5
WALL, NR = 256, 1024
DR = 1.28 / NR
R0 = (NR // 8) * DR
WAVELENGTH = 4.0 / WALL          # four wall-point spacings: P = 6.25 bins


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phasor_bp.json"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--power", type=int, default=0)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--label", default="", help="names the build that was timed (A/B runs)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_phasor needs a GPU"
    g = torch.Generator().manual_seed(0)
    walls = relay_wall_grid(WALL, WALL, device=DEV)
    nmeas = WALL * WALL
    rows = torch.rand(nmeas, NR, generator=g).to(DEV)
    kernel = phasor_kernel(WAVELENGTH, DR, 4.0)
    rows_c = phasor_rows(rows, kernel)                               # [nmeas, NR, 2]: 537 MB
    re, im = rows_c[..., 0].contiguous(), rows_c[..., 1].contiguous()
    filt = timed_alternating({"phasor_rows": lambda: phasor_rows(rows, kernel)}, a.warmup, a.repeats)
    lasers = {"confocal": None,
              "per_meas": (walls + torch.tensor([0.1, 0.0, 0.05], device=DEV)).contiguous(),
              "one_laser": torch.tensor([[0.1, 0.0, -0.2]], device=DEV)}
    n = a.res
    grid = VoxelGrid(POS, SIZE, n)
    planes, mag = torch.empty((2,) + grid.shape, device=DEV), None
    o_re, o_im, o_mag = (torch.empty(grid.shape, device=DEV) for _ in range(3))
    res = {"workload": f"{WALL} x {WALL} wall (extent 1 at y = 0), {NR} bins of c deltaT = 1.28 / {NR} from bin {NR // 8} "
                       f"(C3's window), uniform-random rows (seed 0) filtered with the Morlet wavelet of wavelength "
                       f"{WAVELENGTH} ({len(kernel[0])} taps); volume {SIZE} at {POS}, {n}^3 voxels; power {a.power}",
           "device": torch.cuda.get_device_name(0), "label": a.label,
           "timing": "fused and composed alternating, device events around each call, median of the rounds",
           "fused": "phasor_backproject (planes and magnitude in one kernel)",
           "composed": "backproject(re) + backproject(im) + torch.hypot",
           "phasor_rows": dict(stats(filt["phasor_rows"]), taps=len(kernel[0])), "cases": {}}
    for name, las in lasers.items():
        def fused():
            phasor_backproject(rows_c, walls, grid, R0, DR, power=a.power, lasers=las, planes=planes)

        def composed():
            backproject(re, walls, grid, R0, DR, power=a.power, out=o_re, lasers=las)
            backproject(im, walls, grid, R0, DR, power=a.power, out=o_im, lasers=las)
            torch.hypot(o_re, o_im, out=o_mag)

        ms = timed_alternating({"fused": fused, "composed": composed}, a.warmup, a.repeats)
        _, mag = phasor_backproject(rows_c, walls, grid, R0, DR, power=a.power, lasers=las, planes=planes)
        composed()
        torch.cuda.synchronize()
        e = {"fused": stats(ms["fused"]), "composed": stats(ms["composed"]),
             "planes_bitwise_equal": bool(torch.equal(planes[0], o_re) and torch.equal(planes[1], o_im)),
             "mag_max_rel_diff_vs_hypot": float(((mag - o_mag).abs() / o_mag.clamp_min(1e-30)).max()),
             "pairs": n ** 3 * nmeas}
        e["fused_over_composed"] = e["fused"]["median_ms"] / e["composed"]["median_ms"]
        e["pairs_per_s_fused"] = e["pairs"] / (e["fused"]["median_ms"] * 1e-3)
        res["cases"][name] = e
        print(name, e, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": f"phasor gather {n}^3 x {WALL}^2 x {NR}: fused / composed (worst of three cases)",
                      "value": max(c["fused_over_composed"] for c in res["cases"].values())}))


if __name__ == "__main__":
    main()
