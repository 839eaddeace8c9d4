"""CPU estimate of what NLOSGR_FLAG_FX_TRIM drops from the no-occlusion FX forward (csrc/nlosgr_volume.hpp,
fx_trim_m2): every (wall point, Gaussian) pair's support ends where its value falls under a quarter of the drain's
unit 2^-E, when that radius is inside the cutoff, and a pair that peaks under a quarter unit is skipped.

For a sample of pairs it evaluates, in float64, the kernel's box and support formulas (nlosgr/enum_replay.py) twice,
at the cutoff and at each pair's radius m^2 = min(m_c^2, 2 ln 2 (lw + 2 + 2^-6)), lw = log2(sigma rho 2^E), with the
oracle's albedo rho and the kernel's unit rule (E from the ceil(Ng / 256)-th largest amplitude bound's binary
exponent, over ALL the scene's Gaussians), and prints pairs, dead pairs, rays, in-support bins, box cells, queue
entries (run pairing, groups of two), enumeration trips and lane-rounds at the twin drain's round length, kept and
dropped.

    python scripts/trim_estimate.py [--scene c3|small] [--gaussians 3000] [--walls 6] [--steps 36]

--scene c3: the seeded C3 scene of bench.py (100 000 Gaussians, 128 x 128 wall, 1024 bins, ns 32), a sample of
Gaussians x wall points.  --scene small: the 1500 Gaussians, 3 x 3 wall, 256 bins, ns 16 of tests/test_gpu_fx_trim.py,
every pair, to set against the counting build (scripts/fx_counts.py given small trim: rays_taken, pairs_dropped).
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)

FX_BITS = 24                 # kFxBits
K_TRIM = 2.0 * math.log(2.0)  # kTrim
QUARTER = 2.0 + 2.0 ** -6    # kTrimQuarter


def unit_exponent(m):
    """E of fx_unit_kernel for the whole scene (cuda preset, no occlusion): bounds sigma (0.5 + 1.05 sum_l |f_l|
    sqrt((2l + 1) / 4 pi)) 1.001, E = kFxBits - (binary exponent of the ceil(n / 256)-th largest bound)."""
    import torch
    with torch.no_grad():
        f = torch.cat([m._features_dc, m._features_rest], 1)[:, :, 0].double()
        deg = min(int(m.active_sh_degree), 3)
        sh = sum(f[:, l * l:(l + 1) * (l + 1)].norm(dim=1) * ((2 * l + 1) / (4 * math.pi)) ** 0.5 for l in range(deg + 1))
        b = (torch.sigmoid(m._opacity.double()).reshape(-1) * (0.5 + 1.05 * sh) * 1.001).numpy()
    e = np.floor(np.log2(b[b > 0])).astype(np.int64) + 1        # b in [2^(e-1), 2^e)
    kq = (len(e) + 255) // 256
    return FX_BITS - int(np.sort(e)[::-1][kq - 1])


def tally(E_, box, ok, kl, kh, live, steps):
    t = dict(pairs=0, rays=0, bins=0, cells=0, entries=0, trips=0, rounds=0)
    for g in np.nonzero(ok.any((1, 2)) & live)[0]:
        i0, i1, j0, j1 = box[g]
        okb = ok[g, i0:i1 + 1, j0:j1 + 1]
        klb, khb = kl[g, i0:i1 + 1, j0:j1 + 1], kh[g, i0:i1 + 1, j0:j1 + 1]
        grp, _, ntr = E_.groups_run(okb, 2)
        t["pairs"] += 1
        t["rays"] += int(okb.sum())
        t["bins"] += int((khb - klb + 1)[okb].sum())
        t["cells"] += okb.size
        t["entries"] += len(grp)
        t["trips"] += ntr
        t["rounds"] += E_.lane_rounds(grp, klb, khb, steps)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("c3", "small"), default="c3")
    ap.add_argument("--gaussians", type=int, default=3000)
    ap.add_argument("--walls", type=int, default=6)
    ap.add_argument("--steps", type=int, default=36, help="bins per round of the twin drain")
    ap.add_argument("--cutoff", type=float, default=5.7)
    a = ap.parse_args()
    import torch
    from nlosgr import enum_replay as E_
    from nlosgr.model import GaussianParams
    from nlosgr.volume import Scene
    from oracle import torch_ref as R
    if a.scene == "small":
        ng, scene, seed = 1500, Scene(H=3, W=3, T=256, ns=16), 21
    else:
        ng, scene, seed = 100000, Scene(H=128, W=128, T=1024, ns=32), 0
    m = GaussianParams.synthetic(ng, 3, preset="cuda", device="cpu", seed=seed)
    geo = scene.geometry("cpu", "cuda", "noocl")
    E = unit_exponent(m)
    rng = np.random.default_rng(0)
    if a.scene == "small":
        gs, ps = np.arange(ng), np.arange(geo.nwall)
    else:
        gs = np.sort(rng.choice(ng, a.gaussians, replace=False))
        ps = rng.choice(geo.nwall, a.walls, replace=False)
    sub = lambda t: t.detach()[gs]
    Pm = R.Params(sub(m._mu), sub(m._scaling), sub(m._rotation), sub(m._opacity), sub(m._features_dc),
                  sub(m._features_rest), int(m.active_sh_degree), requires_grad=False)
    mu = sub(m._mu).numpy().astype(np.float64)
    A, smax = E_.gaussian_frames(mu, sub(m._scaling).numpy(), sub(m._rotation).numpy())
    sig = torch.sigmoid(sub(m._opacity).double()).reshape(-1).numpy()
    keys = ("pairs", "rays", "bins", "cells", "entries", "trips", "rounds")
    full, trim = dict.fromkeys(keys, 0), dict.fromkeys(keys, 0)
    dead = 0
    lws = []
    for p in ps:
        rho = R.albedo(Pm, geo.wall[int(p)].float(), preset="cuda")[:, 0].double().numpy()
        live = rho > 0
        with np.errstate(divide="ignore"):
            lw = np.log2(np.where(live, sig * rho, 1.0)) + E
        m2 = np.minimum(a.cutoff ** 2, K_TRIM * (lw + QUARTER))
        alive = live & (m2 > 0)
        box, ok, kl, kh = E_.wall_point_cells(geo, int(p), mu, A, smax, a.cutoff)
        tf = tally(E_, box, ok, kl, kh, live, a.steps)
        dead += int((ok.any((1, 2)) & live & ~alive).sum())
        lws.append(lw[ok.any((1, 2)) & live])
        box, ok, kl, kh = E_.wall_point_cells(geo, int(p), mu, A, smax, np.sqrt(np.maximum(m2, 0.0)))
        tt = tally(E_, box, ok, kl, kh, alive, a.steps)
        for k in keys:
            full[k] += tf[k]
            trim[k] += tt[k]
    lws = np.concatenate(lws)
    print(f"scene {a.scene}: {len(gs)} Gaussians x {len(ps)} wall points, E {E}; lw of the pairs in support: median "
          f"{np.median(lws):.2f}, 10 % {np.quantile(lws, 0.1):.2f}, 90 % {np.quantile(lws, 0.9):.2f}; pairs whose "
          f"radius is inside the cutoff {float((K_TRIM * (lws + QUARTER) < a.cutoff ** 2).mean()):.3f}")
    print(f"{'':>10} {'full':>12} {'trimmed':>12} {'kept':>7}")
    for k in keys:
        print(f"{k:>10} {full[k]:>12} {trim[k]:>12} {trim[k] / max(full[k], 1):>7.3f}")
    print(f"dead pairs (peak under a quarter unit): {dead} of {full['pairs']}; bins per ray {full['bins'] / max(full['rays'], 1):.1f} "
          f"-> {trim['bins'] / max(trim['rays'], 1):.1f}")


if __name__ == "__main__":
    main()
