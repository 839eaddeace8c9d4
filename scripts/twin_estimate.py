"""CPU replay of the forward's segment geometry: what the twin drain (csrc/nlosgr_volume.hip, fx_twin_setup)
can save at a benchmark configuration.

For a sample of (wall point, Gaussian) pairs of the seeded C3 scene it evaluates the kernel's own support
formulas in float64 (ray_setup: closest approach, m2min, [kl, kh]), walks each pair's candidate box in
row-major trips of NC cells as enumerate_box does, pairs two passing cells (i, j), (i, j + 1) of one trip, and
reports
  * rays per pair and bins per segment (to compare with the profile's 26.7 / 66.0 at C3, 5.7 sigma),
  * the fraction of rays that find a twin, the union length against the two lengths, the distance of the
    two closest-approach bins,
  * lane-rounds (= ds_add_u64 instructions / (kSteps / 2)) and segments taken at refills, single vs twin.

    python scripts/twin_estimate.py [--nc 3] [--gaussians 300] [--walls 8] [--steps 28]
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))


def rot(q):
    r, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nc", type=int, default=3, help="candidate cells per enumeration trip")
    ap.add_argument("--gaussians", type=int, default=300)
    ap.add_argument("--walls", type=int, default=8)
    ap.add_argument("--steps", type=int, default=28, help="bins per drain round (NLOSGR_FSTEPS)")
    ap.add_argument("--cutoff", type=float, default=5.7)
    a = ap.parse_args()
    from nlosgr.model import GaussianParams
    from nlosgr.volume import Scene
    ng, H, T, ns = 100000, 128, 1024, 32
    scene = Scene(H=H, W=H, T=T, ns=ns)
    m = GaussianParams.synthetic(ng, 3, preset="cuda", device="cpu", seed=0)
    geo = scene.geometry("cpu", "cuda", "noocl")
    rng = np.random.default_rng(0)
    gs = rng.choice(ng, a.gaussians, replace=False)
    ps = rng.choice(H * H, a.walls, replace=False)
    mu = m._mu.detach().numpy().astype(np.float64)
    sc = np.exp(m._scaling.detach().numpy().astype(np.float64))
    q = m._rotation.detach().numpy().astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    r = geo.r.numpy().astype(np.float64)
    nr = len(r)
    r0, dr = r[0], (r[-1] - r[0]) / (nr - 1)
    mc2 = a.cutoff ** 2
    S = a.steps

    def rounds(l0, l1):   # rounds start at the even bin at or below the first bin
        return math.ceil((l1 - l0 + 1 + (int(l0) & 1)) / S)

    rays = pairs = twinned = 0
    len_sum = union_sum = twin_len_sum = 0.0
    rounds_single = rounds_twin = 0
    dks = []
    for p in ps:
        st, ct = (geo.sin_theta[p].numpy().astype(np.float64), geo.cos_theta[p].numpy().astype(np.float64))
        sp, cp = (geo.sin_phi[p].numpy().astype(np.float64), geo.cos_phi[p].numpy().astype(np.float64))
        D = np.stack([st[:, None] * cp[None, :], st[:, None] * sp[None, :],
                      np.broadcast_to(ct[:, None], (ns, ns))], axis=-1)
        w = geo.wall[p].numpy().astype(np.float64)
        for g in gs:
            A = np.diag(1 / sc[g]) @ rot(q[g]).T
            u0 = A @ (w - mu[g])
            V = D @ A.T
            av = (V * V).sum(-1)
            uv = V @ u0
            ts = -uv / av
            m2 = (u0 @ u0) - uv * uv / av
            ks = (ts - r0) / dr
            hk = np.sqrt(np.maximum(mc2 - m2, 0) / av) / dr
            kl = np.maximum(np.ceil(ks - hk), 0)
            kh = np.minimum(np.floor(ks + hk), nr - 1)
            ok = (m2 <= mc2) & (kl <= kh)
            if not ok.any():
                continue
            pairs += 1
            ii, jj = np.where(ok)   # the candidate box: the passing cells and one row / column of margin
            i0, i1 = max(ii.min() - 1, 0), min(ii.max() + 1, ns - 1)
            j0, j1 = max(jj.min() - 1, 0), min(jj.max() + 1, ns - 1)
            cells = [(i, j) for i in range(i0, i1 + 1) for j in range(j0, j1 + 1)]
            for c0 in range(0, len(cells), a.nc):
                trip = cells[c0:c0 + a.nc]
                u = 0
                while u < len(trip):
                    i, j = trip[u]
                    if not ok[i, j]:
                        u += 1
                        continue
                    rays += 1
                    L = kh[i, j] - kl[i, j] + 1
                    len_sum += L
                    rs = rounds(kl[i, j], kh[i, j])
                    rounds_single += rs
                    if u + 1 < len(trip) and trip[u + 1] == (i, j + 1) and ok[i, j + 1]:
                        rays += 1
                        L2 = kh[i, j + 1] - kl[i, j + 1] + 1
                        len_sum += L2
                        rounds_single += rounds(kl[i, j + 1], kh[i, j + 1])
                        ul, uh = min(kl[i, j], kl[i, j + 1]), max(kh[i, j], kh[i, j + 1])
                        twinned += 2
                        union_sum += uh - ul + 1
                        twin_len_sum += L + L2
                        rounds_twin += rounds(ul, uh)
                        dks.append(abs(ks[i, j] - ks[i, j + 1]))
                        u += 2
                    else:
                        rounds_twin += rs
                        u += 1
    print(f"NC {a.nc}: {pairs} pairs, {rays / pairs:.1f} rays per pair, {len_sum / rays:.1f} bins per segment")
    print(f"twinned rays {twinned / rays:.3f}; union / mean of the two lengths "
          f"{2 * union_sum / max(twin_len_sum, 1):.3f}; closest-approach bins apart mean {np.mean(dks):.1f} "
          f"max {np.max(dks):.1f}")
    print(f"lane-rounds single {rounds_single}, with twins {rounds_twin}: x{rounds_twin / rounds_single:.3f}")
    print(f"segments taken at refills single {rays}, with twins {rays - twinned // 2}: "
          f"x{(rays - twinned // 2) / rays:.3f}")


if __name__ == "__main__":
    main()
