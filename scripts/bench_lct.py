"""Light-cone transform timing at 128 x 128 wall points x 1024 bins, nv = 1024 (work arrays 256 x 256 x 2048
complex64, 1 GiB): each stage (load, FFT, kernel, the inverse, the Wiener product, inverse FFT, store) and the whole
lct_reconstruct, with the inverse built in the call and with it passed in, against
  - the same definition as a torch composition: dense R matmuls on both sides, pad, fftn, an elementwise product with
    the inverse, ifftn, clamp, permute (R, the radial weights and the inverse depend on the geometry alone and are
    built outside the timed region, so it is compared with lct_reconstruct(inverse=)), and
  - fk_migrate on the same rows.
The variants alternate in one process, the median after a warm-up; a stage is timed as --inner back-to-back calls
between two device events, a whole reconstruction as one call (bench_fk.py's method).  For each kernel the achieved
bytes per second against its minimum traffic (computed here from the shapes) is reported, and the share of the FFTs
in each total.  Writes one JSON file.

    python scripts/bench_lct.py [--out profiles/lct_c3.json] [--repeats 10] [--wall 128] [--nr 1024] [--nv 1024]
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
from nlosgr import fk as FK  # noqa: E402
from nlosgr import lct as LCT  # noqa: E402

DEV = torch.device("cuda:0")


class TorchLct:
    """The definition of include/nlosgr.h as torch calls; R (dense, fp32), the radial weights and the inverse are
    built once."""

    def __init__(self, H, W, res, inverse, r0, dr, power=4):
        self.H, self.W, self.nr, self.nv = H, W, res.nr, res.nv
        self.R = res.dense().float().to(DEV)                                     # [nv, nr]
        self.Rt = self.R.t().contiguous()
        r = float(np.float32(r0)) + float(np.float32(dr)) * torch.arange(res.nr, dtype=torch.float64)
        self.w = (r ** power).float().to(DEV)
        self.G = inverse

    def __call__(self, rows):
        H, W, nv = self.H, self.W, self.nv
        g = (rows.clamp_min(0.0) * self.w[None, :]) @ self.Rt                    # [H W, nv]
        pad = torch.zeros(2 * H, 2 * W, 2 * nv, device=DEV)
        pad[:H, :W, :nv] = g.reshape(H, W, nv)
        o = torch.fft.ifftn(torch.fft.fftn(pad) * self.G)
        return (o[:H, :W, :nv].real @ self.R).clamp_min(0.0).permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lct_c3.json"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls between the events of a stage timing")
    ap.add_argument("--wall", type=int, default=128)
    ap.add_argument("--nr", type=int, default=1024)
    ap.add_argument("--nv", type=int, default=None, help="depth-squared cells (default: nr)")
    ap.add_argument("--snr", type=float, default=0.8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lct needs a GPU"
    H = W = a.wall
    nr = a.nr
    dr = 1.28 / 1024
    I1 = nr // 8
    r0 = I1 * dr
    sx = sz = 1.0 / a.wall
    g = torch.Generator().manual_seed(0)
    rows = torch.rand(H * W, nr, generator=g).to(DEV)

    res = LCT.lct_resampling(r0, dr, nr, a.nv)
    nv = res.nv
    pad = LCT.lct_load(rows, H, W, r0, dr, resampling=res)
    spec = torch.fft.fftn(pad)
    K = LCT.lct_kernel(H, W, nv, sx, sz, res.dv)
    kf = torch.fft.fftn(K)
    G = LCT.lct_filter(None, kf=kf, snr=a.snr)
    prod = LCT.lct_filter(spec, inverse=G)
    field = torch.fft.ifftn(prod)
    stages = {
        "load": lambda: LCT.lct_load(rows, H, W, r0, dr, resampling=res, out=pad),
        "fft": lambda: torch.fft.fftn(pad),
        "kernel": lambda: LCT.lct_kernel(H, W, nv, sx, sz, res.dv, out=K),
        "inverse": lambda: LCT.lct_filter(None, kf=kf, snr=a.snr, out=G),
        "product": lambda: LCT.lct_filter(spec, inverse=G, out=prod),
        "ifft": lambda: torch.fft.ifftn(prod),
        "store": lambda: LCT.lct_store(field, res),
    }
    ms = timed_alternating(stages, a.warmup, a.repeats, inner=a.inner)
    A = 8 * (2 * H) * (2 * W) * (2 * nv)                    # bytes of a work array
    traffic = {"load": 4 * H * W * nr + A,                  # the rows once, the padded array once
               "kernel": A,                                 # written once
               "inverse": 2 * A,                            # one spectrum read, one written
               "product": 3 * A,                            # two spectra read, one written
               "store": A // 8 + 4 * H * W * nr}            # the [0:H, 0:W, 0:nv] corner, the volume
    out = {"workload": f"{H} x {W} wall (spacing 1 / {a.wall}), {nr} bins of c deltaT = 1.28 / 1024 from bin {I1}, "
                       f"nv = {nv} cells, snr {a.snr:g}, power 4, uniform-random rows (seed 0); work arrays {2 * H} x "
                       f"{2 * W} x {2 * nv} complex64 ({A / 2 ** 30:.3g} GiB); resampling tables of {res.nnz} weights",
           "device": torch.cuda.get_device_name(0),
           "timing": f"variants alternating in one process, median of the rounds; stages: device events around {a.inner} "
                     "back-to-back calls, time per call; totals: device events around one call",
           "stages": {k: stats(v) for k, v in ms.items()}, "min_traffic_bytes": traffic}
    for k, nbytes in traffic.items():
        out["stages"][k]["achieved_TB_per_s"] = nbytes / (out["stages"][k]["median_ms"] * 1e-3) / 1e12
    del pad, spec, K, kf, prod, field

    tl = TorchLct(H, W, res, G, r0, dr)
    totals = timed_alternating({
        "lct_reconstruct": lambda: LCT.lct_reconstruct(rows, H, W, sx, sz, r0, dr, snr=a.snr, nv=a.nv),
        "lct_reconstruct_inverse_given": lambda: LCT.lct_reconstruct(rows, H, W, sx, sz, r0, dr, nv=a.nv, inverse=G),
        "torch_composition_inverse_given": lambda: tl(rows),
        "fk_migrate": lambda: FK.fk_migrate(rows, H, W, sx, sz, r0, dr),
    }, a.warmup, a.repeats)
    out["totals"] = {k: stats(v) for k, v in totals.items()}
    got, want = LCT.lct_reconstruct(rows, H, W, sx, sz, r0, dr, nv=a.nv, inverse=G), tl(rows)
    out["max_diff_vs_torch_composition_of_max"] = float((got - want).abs().max() / want.max())
    out["bitwise_repeatable"] = bool(torch.equal(got, LCT.lct_reconstruct(rows, H, W, sx, sz, r0, dr, nv=a.nv, inverse=G)))
    out["inverse_given_equals_built"] = bool(torch.equal(got, LCT.lct_reconstruct(rows, H, W, sx, sz, r0, dr,
                                                                                 snr=a.snr, nv=a.nv)))
    st = out["stages"]
    kern = sum(st[k]["median_ms"] for k in ("load", "product", "store"))
    ffts = st["fft"]["median_ms"] + st["ifft"]["median_ms"]
    build = st["kernel"]["median_ms"] + st["fft"]["median_ms"] + st["inverse"]["median_ms"]
    given = out["totals"]["lct_reconstruct_inverse_given"]["median_ms"]
    total = out["totals"]["lct_reconstruct"]["median_ms"]
    out["shares_of_total"] = {
        "inverse_given": {"kernels_ms": kern, "ffts_ms": ffts, "total_ms": given, "kernels": kern / given,
                          "ffts": ffts / given},
        "inverse_built": {"kernels_ms": kern + st["kernel"]["median_ms"] + st["inverse"]["median_ms"],
                          "ffts_ms": ffts + st["fft"]["median_ms"], "building_the_inverse_ms": build, "total_ms": total,
                          "kernels": (kern + st["kernel"]["median_ms"] + st["inverse"]["median_ms"]) / total,
                          "ffts": (ffts + st["fft"]["median_ms"]) / total}}
    out["lct_inverse_given_over_torch_composition"] = given / out["totals"]["torch_composition_inverse_given"]["median_ms"]
    out["lct_inverse_given_over_fk_migrate"] = given / out["totals"]["fk_migrate"]["median_ms"]
    out["lct_over_fk_migrate"] = total / out["totals"]["fk_migrate"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))
    print(json.dumps({"metric": f"light-cone transform {H} x {W} x {nr}: total ms", "value": total}))


if __name__ == "__main__":
    main()
