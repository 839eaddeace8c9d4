"""CPU replay of the forward's enumeration and segment geometry: what grouping adjacent rays into one lane
(csrc/nlosgr_volume_fwd.hip, enumerate_runs and fx_twin_setup) saves at a benchmark configuration.

For a sample of (wall point, Gaussian) pairs of the seeded C3 scene it evaluates, in float64, the kernel's own
bounding-sphere box (pair_setup) and support formulas (ray_setup: closest approach, m2min, [kl, kh]) through
nlosgr/enum_replay.py, groups each box's passing cells the way the chosen scheme does and reports
  * rays, box cells and rows per pair, passing cells per row, rows whose passing cells are not contiguous,
  * cells tested and trips (the enumeration's own work),
  * queue entries per ray and the share of rays in groups of two or more,
  * lane-rounds (= ds_add_u64 instructions / (round length / 2)) at the given round length, against the
    one-ray-per-lane drain at 28-bin rounds.

    python scripts/twin_estimate.py [--pairing trip|run] [--group 2|3] [--steps 36] [--gaussians 400] [--walls 6]

--pairing trip: row-major trips of 3 cells that wrap across rows, two adjacent passing cells of a trip pair up
(the scheme before enumerate_runs; --group 2 only).  --pairing run: trips of 4 cells of one row, trip_plan of
csrc/nlosgr_enum.hpp.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairing", choices=("trip", "run"), default="run")
    ap.add_argument("--group", type=int, choices=(2, 3), default=2, help="rays per lane at most (K)")
    ap.add_argument("--gaussians", type=int, default=400)
    ap.add_argument("--walls", type=int, default=6)
    ap.add_argument("--steps", type=int, default=36, help="bins per drain round of the grouped drain")
    ap.add_argument("--single-steps", type=int, default=28, help="bins per round of the one-ray-per-lane drain")
    ap.add_argument("--cutoff", type=float, default=5.7)
    a = ap.parse_args()
    if a.pairing == "trip" and a.group != 2:
        ap.error("--pairing trip forms pairs only")
    from nlosgr import enum_replay as E
    from nlosgr.model import GaussianParams
    from nlosgr.volume import Scene
    from oracle import torch_ref as R
    ng, H, T, ns = 100000, 128, 1024, 32
    scene = Scene(H=H, W=H, T=T, ns=ns)
    m = GaussianParams.synthetic(ng, 3, preset="cuda", device="cpu", seed=0)
    geo = scene.geometry("cpu", "cuda", "noocl")
    rng = np.random.default_rng(0)
    gs = np.sort(rng.choice(ng, a.gaussians, replace=False))
    ps = rng.choice(H * H, a.walls, replace=False)
    sub = lambda t: t.detach()[gs]
    Pm = R.Params(sub(m._mu), sub(m._scaling), sub(m._rotation), sub(m._opacity), sub(m._features_dc),
                  sub(m._features_rest), int(m.active_sh_degree), requires_grad=False)
    mu = sub(m._mu).numpy().astype(np.float64)
    A, smax = E.gaussian_frames(mu, sub(m._scaling).numpy(), sub(m._rotation).numpy())

    pairs = rays = cells = rows = prow = noncontig = tested = trips = entries = grouped = 0
    rounds = rounds_single = 0
    for p in ps:
        box, ok, kl, kh = E.wall_point_cells(geo, int(p), mu, A, smax, a.cutoff)
        rho = R.albedo(Pm, geo.wall[int(p)].float(), preset="cuda")[:, 0].numpy()
        ok &= (rho > 0)[:, None, None]
        for g in np.nonzero(ok.any((1, 2)))[0]:
            i0, i1, j0, j1 = box[g]
            okb = ok[g, i0:i1 + 1, j0:j1 + 1]
            klb, khb = kl[g, i0:i1 + 1, j0:j1 + 1], kh[g, i0:i1 + 1, j0:j1 + 1]
            pairs += 1
            rays += int(okb.sum())
            cells += okb.size
            live = okb.any(1)
            rows += int(live.sum())
            for row in okb[live]:
                idx = np.nonzero(row)[0]
                prow += len(idx)
                noncontig += int(idx[-1] - idx[0] + 1 != len(idx))
            grp, nt_, ntr = E.groups_trip(okb) if a.pairing == "trip" else E.groups_run(okb, a.group)
            tested += nt_
            trips += ntr
            entries += len(grp)
            grouped += sum(l for _, _, l in grp if l > 1)
            rounds += E.lane_rounds(grp, klb, khb, a.steps)
            singles = [(i, j, 1) for i, j in zip(*np.nonzero(okb))]
            rounds_single += E.lane_rounds(singles, klb, khb, a.single_steps)
    print(f"{a.gaussians} Gaussians x {a.walls} wall points: {pairs} pairs, {rays} rays; per pair {rays / pairs:.1f} "
          f"rays, {cells / pairs:.1f} box cells, {rows / pairs:.1f} rows; {prow / rows:.1f} passing cells per row, "
          f"{noncontig} rows not contiguous")
    print(f"pairing {a.pairing}, K {a.group}: cells tested {tested}, trips {trips}; entries per ray "
          f"{entries / rays:.3f}; rays in groups {grouped / rays:.3f}")
    at = rounds * a.steps
    at1 = rounds_single * a.single_steps
    print(f"lane-rounds at {a.steps} bins {rounds} (one ray per lane at {a.single_steps} bins: {rounds_single}); "
          f"atomics (lane-rounds x bins per round) vs the one-ray drain x{at / at1:.3f}")


if __name__ == "__main__":
    main()
