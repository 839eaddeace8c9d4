"""Fast phasor field (nlosgr.rsd) timing at a 128 x 128 wall x 1024 bins, 128 depth planes, a wavelength of 4 wall
spacings, confocal and with one laser spot: each stage (rfft, load, the image FFT; per chunk of depth planes kernel,
fft2, apply, ifft2, gather), the FFTs' share, the whole rsd_reconstruct, and beside it what phasor_capture does on the
same voxels: phasor_rows + phasor_backproject (the brute-force gather over every voxel-measurement pair).
The variants alternate in one process, the median after a warm-up; a stage is timed as --inner back-to-back calls
between two device events, a whole reconstruction as one call.  Per-chunk stages are timed on one full chunk and
reported per reconstruction (times the planes, over the chunk's planes).  For each kernel the achieved bytes per
second against its minimum traffic (computed here from the shapes) is reported.  Writes one JSON file.

    python scripts/bench_rsd.py [--out profiles/rsd_c3.json] [--repeats 10] [--wall 128] [--nr 1024] [--planes 128]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nlosgr import rsd as R  # noqa: E402
from nlosgr.fk import lattice_spacing  # noqa: E402
from nlosgr.geometry import relay_wall_grid  # noqa: E402
from nlosgr.phasor import phasor_backproject, phasor_kernel, phasor_rows  # noqa: E402
from nlosgr.voxelize import VoxelGrid  # noqa: E402

DEV = torch.device("cuda:0")
LASER = (0.1, 0.0, -0.2)


def timed_alternating(fns, warmup, repeats, inner=1):
    """{name: [ms per call]}: the variants run in turn, `repeats` rounds, device events around `inner` back-to-back
    calls of one variant."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / inner)
    return out


def stats(ms, scale=1.0):
    s = sorted(v * scale for v in ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "repeats": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rsd_c3.json"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5, help="back-to-back calls between the events of a stage timing")
    ap.add_argument("--wall", type=int, default=128)
    ap.add_argument("--nr", type=int, default=1024)
    ap.add_argument("--planes", type=int, default=128)
    ap.add_argument("--work-bytes", type=int, default=1 << 30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rsd needs a GPU"
    H = W = a.wall
    nr, ny = a.nr, a.planes
    dr = 1.28 / 1024
    I1 = nr // 8
    r0, y0 = I1 * dr, 0.0
    walls = relay_wall_grid(H, W, device=DEV)
    xs, zs = walls[:W, 0].contiguous().cpu(), walls[::W, 2].contiguous().cpu()
    sx, sz = lattice_spacing(xs), lattice_spacing(zs)
    wavelength = 4.0 * sx
    ys = torch.from_numpy(np.linspace(0.25, 0.75, ny).astype(np.float32))
    rows = torch.rand(H * W, nr, generator=torch.Generator().manual_seed(0)).to(DEV)
    grid = VoxelGrid(tables=(xs, ys, zs))
    kernel = phasor_kernel(wavelength, dr)
    res = {"device": torch.cuda.get_device_name(0),
           "timing": f"variants alternating in one process, median of the rounds; stages: device events around {a.inner} "
                     "back-to-back calls, time per call; totals: device events around one call",
           "cases": {}}
    for case, laser in (("confocal", None), ("one_laser", LASER)):
        Nt = R.rsd_nt(nr, xs, zs, y0, ys, r0, dr, wavelength, 4.0, laser)
        q_lo, coef = R.rsd_band(wavelength, dr, Nt, r0)
        nq = len(coef)
        image = nq * 4 * H * W * 8                               # bytes of one depth plane's images
        step = min(ny, max(1, a.work_bytes // image))
        xd, yd, zd = xs.to(DEV), ys.to(DEV), zs.to(DEV)
        spec = torch.fft.rfft(rows, n=Nt)
        Pw = R.rsd_load(spec, H, W, q_lo, coef)
        Pf = torch.fft.fft2(Pw)
        A = torch.empty((step, nq, 2 * H, 2 * W), dtype=torch.complex64, device=DEV)
        B = torch.empty_like(A)
        planes = torch.empty((2, W, ny, H), device=DEV)
        mag = torch.empty((W, ny, H), device=DEV)
        once = {
            "rfft": lambda: torch.fft.rfft(rows, n=Nt),
            "load": lambda: R.rsd_load(spec, H, W, q_lo, coef, out=Pw),
            "image_fft2": lambda: torch.fft.fft2(Pw),
        }
        chunk = {
            "kernel": lambda: R.rsd_kernel(yd, y0, H, W, sx, sz, dr, Nt, q_lo, nq, laser=laser is not None, nj=step, out=A),
            "fft2": lambda: torch.fft.fft2(A, out=B),
            "apply": lambda: R.rsd_apply(B, Pf),
            "ifft2": lambda: torch.fft.ifft2(B, out=A),
            "gather": lambda: R.rsd_gather(A, q_lo, Nt, dr, xd, yd, zd, laser=laser, out=planes, mag=mag),
        }
        ms = timed_alternating({**once, **chunk}, a.warmup, a.repeats, inner=a.inner)
        per = ny / step                                          # chunks per reconstruction (the last may be partial)
        st = {k: stats(ms[k]) for k in once}
        st.update({k: stats(ms[k], per) for k in chunk})
        traffic = {"load": 8 * H * W * nq + image,               # the band of every row once, the padded images once
                   "kernel": image * ny,                         # every kernel image written once
                   "apply": 2 * image * ny + image,              # read and written in place; the image spectrum once
                   "gather": image * ny // 4 + 12 * H * W * ny}  # the [0:H, 0:W] corner; two planes and the magnitude
        for k, nbytes in traffic.items():
            st[k]["achieved_TB_per_s"] = nbytes / (st[k]["median_ms"] * 1e-3) / 1e12
        del A, B, spec, Pw, Pf
        rows_c = phasor_rows(rows, kernel)
        lasers = None if laser is None else torch.tensor([laser], device=DEV)
        totals = timed_alternating({
            "rsd_reconstruct": lambda: R.rsd_reconstruct(rows, H, W, xs, zs, y0, ys, r0, dr, wavelength, laser=laser,
                                                         work_bytes=a.work_bytes),
            "phasor_rows": lambda: phasor_rows(rows, kernel),
            "phasor_backproject": lambda: phasor_backproject(rows_c, walls, grid, r0, dr, lasers=lasers),
        }, a.warmup, a.repeats)
        tot = {k: stats(v) for k, v in totals.items()}
        got = R.rsd_reconstruct(rows, H, W, xs, zs, y0, ys, r0, dr, wavelength, laser=laser, work_bytes=a.work_bytes)
        again = R.rsd_reconstruct(rows, H, W, xs, zs, y0, ys, r0, dr, wavelength, laser=laser, work_bytes=a.work_bytes)
        _, pmag = phasor_backproject(rows_c, walls, grid, r0, dr, lasers=lasers)
        ffts = sum(st[k]["median_ms"] for k in ("rfft", "image_fft2", "fft2", "ifft2"))
        kern = sum(st[k]["median_ms"] for k in ("load", "kernel", "apply", "gather"))
        total = tot["rsd_reconstruct"]["median_ms"]
        gather = tot["phasor_rows"]["median_ms"] + tot["phasor_backproject"]["median_ms"]
        res["cases"][case] = {
            "Nt": Nt, "band": [q_lo, q_lo + nq - 1], "nq": nq, "planes_per_chunk": step, "ffts_2d": (2 * ny + 1) * nq,
            "kernel_elements": ny * nq * 4 * H * W, "gather_pairs": H * W * ny * H * W,
            "stages": st, "min_traffic_bytes": traffic, "totals": tot,
            "shares_of_total": {"kernels_ms": kern, "ffts_ms": ffts, "total_ms": total, "kernels": kern / total,
                                "ffts": ffts / total},
            "phasor_rows_plus_backproject_ms": gather, "rsd_over_phasor_gather": total / gather,
            "bitwise_repeatable": bool(torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])),
            "max_diff_of_normalised_magnitudes_vs_phasor_backproject":
                float((got[1] / got[1].max() - pmag / pmag.max()).abs().max()),
        }
        del rows_c, got, again, pmag, planes, mag
    res["workload"] = (f"{H} x {W} wall (extent 1 at y = 0), {nr} bins of c deltaT = 1.28 / 1024 from bin {I1}, "
                       f"uniform-random rows (seed 0); {ny} depth planes in [0.25, 0.75], wavelength 4 wall spacings, "
                       f"4 cycles; laser spot {LASER} in the one-laser case; work arrays within {a.work_bytes} bytes each")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    print(json.dumps({"metric": f"fast phasor field {H} x {W} x {nr}, {ny} planes, confocal: total ms",
                      "value": res["cases"]["confocal"]["shares_of_total"]["total_ms"]}))


if __name__ == "__main__":
    main()
