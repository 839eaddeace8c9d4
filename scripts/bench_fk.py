"""f-k migration timing at 128 x 128 wall points x 1024 bins (work arrays 256 x 256 x 2048 complex64, 1 GiB): each of
the five stages (load, FFT, Stolt, inverse FFT, store) and the whole fk_migrate, against
  - the same definition as a torch composition: pad, fftn, gather + lerp, ifftn, abs()**2, permute (its index,
    fraction and weight-phase tables depend on the geometry alone and are built outside the timed region), and
  - backproject_capture of the same capture onto 128^3 voxels.
The variants alternate in one process, the median after a warm-up; a stage is timed as --inner back-to-back calls
between two device events (a single sub-millisecond launch would include the host's launch latency), a whole
reconstruction as one call.  The two f-k routes are compared at the timed size.  For each kernel the achieved bytes
per second against its minimum traffic (computed here from the shapes) is reported, and the shares of the kernels and
of the FFTs in the total.  Writes one JSON file.

    python scripts/bench_fk.py [--out profiles/fk_c3.json] [--repeats 10] [--wall 128] [--nr 1024]
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

from nlosgr import fk as FK  # noqa: E402
from nlosgr.backproject import backproject_capture  # noqa: E402
from nlosgr.geometry import relay_wall_grid  # noqa: E402

DEV = torch.device("cuda:0")
POS, SIZE = (0.0, 0.5, 0.0), 0.5


def timed_alternating(fns, warmup, repeats, inner=1):
    """{name: [ms per call]}: the variants run in turn, `repeats` rounds, device events around `inner` back-to-back
    calls of one variant (inner > 1 keeps the queue full, so the host's launch latency, which a single sub-millisecond
    kernel between two events would include, is hidden behind the previous launch)."""
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


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "repeats": len(s)}


def signed(N):
    i = torch.arange(N, device=DEV)
    return torch.where(i < N // 2, i, i - N).double()


class TorchFk:
    """The definition of include/nlosgr.h as torch calls; the Stolt tables are built once, in float64."""

    def __init__(self, H, W, nr, sx, sz, r0, dr):
        self.H, self.W, self.nr = H, W, nr
        Nz, Nx, Nt = 2 * H, 2 * W, 2 * nr
        r0, dr, sx, sz = (float(np.float32(v)) for v in (r0, dr, sx, sz))
        gx, gz = Nt * dr / (Nx * sx), Nt * dr / (Nz * sz)
        a = signed(Nt)[None, None, :]
        src = torch.sqrt(a * a + ((gx * signed(Nx)) ** 2)[None, :, None] + ((gz * signed(Nz)) ** 2)[:, None, None])
        k = torch.floor(src)
        ok = (a > 0) & (k + 1 <= Nt // 2 - 1)
        self.f = torch.where(ok, src - k, torch.zeros_like(src)).float()
        self.k = torch.where(ok, k, torch.zeros_like(k)).long()
        t = (src - a) * (r0 / dr) / Nt
        t = t - torch.floor(t)
        w = torch.where(ok, a / src.clamp_min(1e-300), torch.zeros_like(src))
        self.wphase = torch.polar(w, -2.0 * np.pi * t).to(torch.complex64)
        self.r = (r0 + dr * torch.arange(nr, device=DEV, dtype=torch.float64)).float()
        del src, k, ok, t, w

    def __call__(self, rows, power=4):
        H, W, nr = self.H, self.W, self.nr
        psi = torch.sqrt(rows.clamp_min(0.0) * self.r[None, :] ** power).reshape(H, W, nr)
        pad = torch.zeros(2 * H, 2 * W, 2 * nr, device=DEV)
        pad[:H, :W, :nr] = psi
        S = torch.fft.fftn(pad)
        V = (torch.gather(S, 2, self.k) * (1.0 - self.f) + torch.gather(S, 2, self.k + 1) * self.f) * self.wphase
        o = torch.fft.ifftn(V)
        return (o[:H, :W, :nr].abs() ** 2).permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fk_c3.json"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls between the events of a stage timing")
    ap.add_argument("--wall", type=int, default=128)
    ap.add_argument("--nr", type=int, default=1024)
    ap.add_argument("--res", type=int, default=128, help="voxels per axis of the back-projection compared with")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fk needs a GPU"
    H = W = a.wall
    nr = a.nr
    dr = 1.28 / 1024
    I1 = nr // 8
    r0 = I1 * dr
    sx = sz = 1.0 / a.wall
    g = torch.Generator().manual_seed(0)
    rows = torch.rand(H * W, nr, generator=g).to(DEV)
    walls = relay_wall_grid(H, W, device=DEV)

    pad = FK.fk_load(rows, H, W, r0, dr)
    spec = torch.fft.fftn(pad)
    mig = FK.fk_stolt(spec, sx, sz, r0, dr)
    field = torch.fft.ifftn(mig)
    stages = {
        "load": lambda: FK.fk_load(rows, H, W, r0, dr, out=pad),
        "fft": lambda: torch.fft.fftn(pad),
        "stolt": lambda: FK.fk_stolt(spec, sx, sz, r0, dr, out=mig),
        "ifft": lambda: torch.fft.ifftn(mig),
        "store": lambda: FK.fk_store(field),
    }
    ms = timed_alternating(stages, a.warmup, a.repeats, inner=a.inner)
    A = 8 * (2 * H) * (2 * W) * (2 * nr)                    # bytes of a work array
    traffic = {"load": 4 * H * W * nr + A,                  # the rows once, the padded array once
               "stolt": A // 2 + A,                         # the positive band of every column, the whole result
               "store": A // 8 + 4 * H * W * nr}            # the [0:H, 0:W, 0:nr] corner, the volume
    res = {"workload": f"{H} x {W} wall (extent 1 at y = 0), {nr} bins of c deltaT = 1.28 / 1024 from bin {I1}, "
                       f"uniform-random rows (seed 0); work arrays {2 * H} x {2 * W} x {2 * nr} complex64 ({A / 2 ** 30:.3g} GiB)",
           "device": torch.cuda.get_device_name(0),
           "timing": f"variants alternating in one process, median of the rounds; stages: device events around {a.inner} "
                     "back-to-back calls, time per call; totals: device events around one call",
           "stages": {k: stats(v) for k, v in ms.items()}, "min_traffic_bytes": traffic}
    for k, nbytes in traffic.items():
        res["stages"][k]["achieved_TB_per_s"] = nbytes / (res["stages"][k]["median_ms"] * 1e-3) / 1e12
    # what work arrays of the non-negative temporal frequencies alone would change in the FFTs (only a >= 0 is read
    # from S and only a > 0 is non-zero in V): rfft along time then fft2, and ifft2 then ifft(n = Nt), on the same data
    pad_real = pad.real.contiguous()
    half = mig[:, :, :nr + 1].contiguous()
    del field
    hs = timed_alternating({
        "fft_full": lambda: torch.fft.fftn(pad),
        "fft_half": lambda: torch.fft.fft2(torch.fft.rfft(pad_real, dim=2), dim=(0, 1)),
        "ifft_full": lambda: torch.fft.ifftn(mig),
        "ifft_half": lambda: torch.fft.ifft(torch.fft.ifft2(half, dim=(0, 1)), n=2 * nr, dim=2),
    }, a.warmup, a.repeats, inner=a.inner)
    res["half_spectrum_ffts"] = {k: stats(v) for k, v in hs.items()}
    del pad, spec, mig, pad_real, half

    tfk = TorchFk(H, W, nr, sx, sz, r0, dr)
    dk = {"nlos_data": torch.zeros(I1 + nr, H, W, device=DEV), "camera_grid_positions": walls.t().contiguous(),
          "volume_position": torch.tensor(POS, device=DEV), "volume_size": SIZE, "c": 1.0, "deltaT": dr}
    dk["nlos_data"][I1:] = rows.t().reshape(nr, H, W)
    totals = timed_alternating({
        "fk_migrate": lambda: FK.fk_migrate(rows, H, W, sx, sz, r0, dr),
        "torch_composition": lambda: tfk(rows),
        "backproject_capture": lambda: backproject_capture(dk, a.res, I1, I1 + nr, power=0, filter="log"),
    }, a.warmup, a.repeats)
    res["totals"] = {k: stats(v) for k, v in totals.items()}
    got, want = FK.fk_migrate(rows, H, W, sx, sz, r0, dr), tfk(rows)
    res["max_diff_vs_torch_composition_of_max"] = float((got - want).abs().max() / want.max())
    res["bitwise_repeatable"] = bool(torch.equal(got, FK.fk_migrate(rows, H, W, sx, sz, r0, dr)))
    st = res["stages"]
    kern = sum(st[k]["median_ms"] for k in ("load", "stolt", "store"))
    ffts = st["fft"]["median_ms"] + st["ifft"]["median_ms"]
    total = res["totals"]["fk_migrate"]["median_ms"]
    res["shares_of_total"] = {"kernels_ms": kern, "ffts_ms": ffts, "total_ms": total, "kernels": kern / total,
                              "ffts": ffts / total}
    res["fk_over_torch_composition"] = total / res["totals"]["torch_composition"]["median_ms"]
    res["fk_over_backproject_capture"] = total / res["totals"]["backproject_capture"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    print(json.dumps({"metric": f"f-k migration {H} x {W} x {nr}: total ms", "value": total}))


if __name__ == "__main__":
    main()
