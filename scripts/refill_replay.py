"""CPU replay of the twin drain loop of the no-occlusion FX forward (csrc/nlosgr_volume_fwd.hip, fwd_body with
TW): the queue top-up (enumerate_runs), the refill rule, the drain rounds, the chunk break and the carry-over of
running segments into the next chunk, wave by wave, from the float64 geometry of nlosgr/enum_replay.py.  It
prints, for the waves it replays, the numbers the -DNLOSGR_FXCOUNT build counts per launch
(scripts/fx_counts.py): drain rounds, refills, entries taken, refills taking fewer than 32 entries and refills
after the chunk's enumeration had ended.

    python scripts/refill_replay.py [--scene small|c3] [--rule tail|parent] [--refill 56] [--steps 36]
                                    [--walls N] [--chunks N] [--seed S]

What it models exactly: which lanes are idle at every turn of the loop, what each refill takes, the rounds every
union needs (kStepsTwin bins from the even bin at or below its first bin), split twins going back to the queue.
What it does not: fp32 rounding of the quadric and support tests (a few cells in 10^5 differ), and the merge
guard's amplitude (fx_seed_ok is evaluated with one log2 amplitude for every pair, --lw, in units).
A replay that does not end raises: the loop has a turn limit far above any terminating run.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "nlos-gaussian-renderer_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

K_BLOCK = 256          # threads of a workgroup: 4 waves of 64 pairs per chunk
K_GROUP = 2            # rays per queue entry, at most
HALF_LOG2E = 0.5 * math.log2(math.e)
COUNTERS = ("rounds", "refills", "entries_taken", "refills_under_32", "refills_in_tail")


class Hang(RuntimeError):
    pass


def seed_ok(ga, al, t):
    """fx_seed_ok."""
    return ga * t * t + al >= -100.0 and ga * (2.0 * t + 1.0) <= 120.0


class Pairs:
    """The pairs of one wall point: box [n, 4], passing cells and supports [n, nt, np] (enum_replay.wall_point_cells
    with details), or any arrays of those shapes (the CPU test builds some by hand)."""

    def __init__(self, box, passq, kl, kh, a=None, ks=None, m2=None, dr=1.0, lw=16.0, live=None):
        self.box, self.passq, self.kl, self.kh = box, passq, kl, kh
        self.a, self.ks, self.m2, self.dr, self.lw = a, ks, m2, dr, lw
        self.live = np.ones(len(box), bool) if live is None else live   # w = sigma rho > 0

    def setup(self, g, i, j, twin):
        """fx_twin_setup: (code, first bin, bins) with code 0 none, 1 one ray, 2 twin, 3 split."""
        has = lambda jj: self.kl[g, i, jj] <= self.kh[g, i, jj]
        gota, gotb = has(j), twin and has(j + 1)
        ja, jb = j, j + 1
        if not gota and gotb:
            ja, gota, gotb = jb, True, False
        if not gota:
            return 0, 0, 0
        kl, kh = int(self.kl[g, i, ja]), int(self.kh[g, i, ja])
        if not gotb:
            return 1, kl, kh - kl + 1
        pos, end = min(kl, int(self.kl[g, i, jb])), max(kh, int(self.kh[g, i, jb]))
        if self.a is not None:
            for jj in (ja, jb):
                ga = -HALF_LOG2E * self.a[g, i, jj] * self.dr * self.dr
                al = -HALF_LOG2E * self.m2[g, i, jj] + self.lw
                if not seed_ok(ga, al, pos - self.ks[g, i, jj]):
                    return 3, kl, kh - kl + 1
        return 2, pos, end - pos + 1


def trip_plan(bits, n, cont, K):
    from nlosgr.enum_replay import trip_plan as tp
    return tp(bits, n, cont, K)


def replay_wave(pairs, chunks, rule="tail", refill=56, steps=36, flags=0, trip_cells=4, limit=10_000_000):
    """One wave over its chunks (a list of arrays of <= 64 pair indices; lanes past an array's end hold no pair),
    then the final pass with no pairs.  flags: 1 = queue entries are taken but never set up, 4 = no lane ever
    becomes active (the kernel's diagnostics flags).  Returns the counters, plus entries enumerated, entries
    re-queued by splits, twins and the active lane-rounds."""
    c = dict.fromkeys(COUNTERS + ("enumerated", "requeued", "twins", "active_lane_rounds", "turns"), 0)
    act = np.zeros(64, bool)
    pos = np.zeros(64, np.int64)
    rem = np.zeros(64, np.int64)
    queue = []   # (lane, length, i, j)
    for chunk in list(chunks) + [None]:
        have = chunk is not None
        more = np.zeros(64, bool)
        ci = np.zeros(64, np.int64)
        cj = np.zeros(64, np.int64)
        gs = np.full(64, -1, np.int64)
        if have:
            gs[:len(chunk)] = chunk
            for l in range(len(chunk)):
                g = gs[l]
                i0, i1, j0, j1 = pairs.box[g]
                more[l] = bool(pairs.live[g]) and i0 <= i1 and j0 <= j1
                ci[l], cj[l] = i0, j0
            if flags & 2:
                more[:] = False
        while True:
            c["turns"] += 1
            if c["turns"] > limit:
                raise Hang(f"the drain loop did not end within {limit} turns: {c}, queue {len(queue)}, "
                           f"idle {int((~act).sum())}, enumerating {int(more.sum())}")
            if len(queue) < 64 and more.any():   # enumerate_runs
                while True:
                    put = [[], []]
                    for l in np.nonzero(more)[0]:
                        g = gs[l]
                        _, i1, j0, j1 = pairs.box[g]
                        n = min(trip_cells, j1 - cj[l] + 1)
                        row = pairs.passq[g, ci[l]]
                        bits = sum(1 << u for u in range(n) if row[cj[l] + u])
                        groups, used = trip_plan(bits, n, cj[l] + trip_cells <= j1, K_GROUP)
                        for k, (s, ln) in enumerate(groups):
                            put[k].append((int(l), ln, int(ci[l]), int(cj[l] + s)))
                        if cj[l] + used > j1:
                            cj[l] = j0
                            ci[l] += 1
                        else:
                            cj[l] += used
                        more[l] = ci[l] <= i1
                    for k in range(2):   # group 0 of every lane in lane order, then group 1
                        queue += put[k]
                        c["enumerated"] += len(put[k])
                    if len(queue) >= 64 or not more.any():
                        break
            anymore = bool(more.any())
            idle = np.nonzero(~act)[0]
            nidle, qcount = len(idle), len(queue)
            if rule == "tail":
                go = nidle >= (refill if anymore else min(refill, qcount))
            else:
                go = nidle >= refill or not anymore
            if qcount > 0 and go:
                ntake = min(nidle, qcount)
                c["refills"] += 1
                c["entries_taken"] += ntake
                c["refills_under_32"] += ntake < 32
                c["refills_in_tail"] += not anymore
                taken, queue = queue[:ntake], queue[ntake:]
                for l, (slot, ln, i, j) in zip(idle, taken):
                    if flags & 1:
                        continue
                    code, p0, n = pairs.setup(gs[slot], i, j, ln == 2)
                    if code == 3:
                        queue.append((slot, 1, i, j + 1))
                        c["requeued"] += 1
                    c["twins"] += code == 2
                    if code and not flags & 4:
                        act[l], pos[l], rem[l] = True, p0, n
            if not act.any():
                if not anymore and not queue:
                    break
                continue
            if not anymore and not queue and have:
                break   # next Gaussians; segments carry over
            c["rounds"] += 1
            c["active_lane_rounds"] += int(act.sum())
            adv = steps - (pos & 1)
            pos[act] += adv[act]
            rem[act] -= adv[act]
            act &= rem > 0
    if queue or act.any():
        raise Hang(f"left with {len(queue)} queued entries and {int(act.sum())} active lanes")
    return c


def wave_chunks(ng, nsplit, split, wave):
    """The chunks of one wave of workgroup (p, split): 64 pairs from g_lo + 64 wave, every K_BLOCK."""
    gper = (((ng + nsplit - 1) // nsplit) + 63) & ~63
    lo, hi = split * gper, min(ng, split * gper + gper)
    return [np.arange(b, min(b + 64, hi)) for b in range(lo + 64 * wave, hi, K_BLOCK)]


def fwd_nsplit(ng, nwall, target=131072, most=8):
    """fwd_nsplit of csrc/nlosgr_volume.hip."""
    return max(1, min((target + nwall - 1) // nwall, (ng + 255) // 256, most))


def wall_pairs(geo, p, mu, A, smax, cutoff, live=None, lw=16.0):
    from nlosgr import enum_replay as E
    box, _, kl, kh, d = E.wall_point_cells(geo, p, mu, A, smax, cutoff, details=True)
    return Pairs(box, d["pass"], kl, kh, d["a"], d["ks"], d["m2"], d["dr"], lw, live)


def replay_scene(geo, mu, log_scaling, rotation, cutoff=5.7, walls=None, waves=None, max_chunks=None, live=None,
                 **kw):
    """Sum of replay_wave over the chosen wall points (default all) and (split, wave) pairs (default all).  live:
    which pairs have a weight sigma rho > 0 (the others are never enumerated), an array [n] or a function of the
    wall point; default all."""
    from nlosgr import enum_replay as E
    A, smax = E.gaussian_frames(mu, log_scaling, rotation)
    ng = len(mu)
    nsp = fwd_nsplit(ng, geo.nwall)
    tot = {}
    lw = kw.pop("lw", 16.0)
    wl = [(s, w) for s in range(nsp) for w in range(4)] if waves is None else waves
    chunks = [wave_chunks(ng, nsp, sp, w)[:max_chunks] for sp, w in wl]
    # only the Gaussians of the replayed chunks are set up (C3: 100 000 Gaussians x 1024 cells per wall point)
    idx = np.unique(np.concatenate([c for ch in chunks for c in ch] + [np.zeros(0, np.int64)])).astype(np.int64)
    for p in (range(geo.nwall) if walls is None else walls):
        lv = live(p) if callable(live) else live
        pairs = wall_pairs(geo, p, mu[idx], A[idx], smax[idx], cutoff, None if lv is None else np.asarray(lv)[idx], lw)
        for ch in chunks:
            c = replay_wave(pairs, [np.searchsorted(idx, x) for x in ch], **kw)
            for k, v in c.items():
                tot[k] = tot.get(k, 0) + int(v)
    return tot


def main():
    import torch
    from nlosgr import GaussianParams
    from nlosgr.train import slab_order, wall_centroid
    from nlosgr.volume import Scene
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="small", choices=("small", "c3"))
    ap.add_argument("--rule", default="tail", choices=("tail", "parent"))
    ap.add_argument("--refill", type=int, default=56)
    ap.add_argument("--steps", type=int, default=36)
    ap.add_argument("--walls", type=int, default=0, help="wall points replayed (0: all of small, 4 of c3)")
    ap.add_argument("--waves", type=int, default=0, help="(split, wave) pairs per wall point (0: all of small, 3 of c3)")
    ap.add_argument("--chunks", type=int, default=0, help="chunks per wave (0: all of small, 6 of c3)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lw", type=float, default=16.0, help="log2 amplitude of every pair, for the merge guard")
    a = ap.parse_args()
    dev = torch.device("cpu")
    if a.scene == "small":
        scene, ng, mseed = Scene(H=3, W=3, T=256, ns=16), 1500, 21
    else:
        scene, ng, mseed = Scene(H=128, W=128, T=1024, ns=32), 100_000, 0
    m = GaussianParams.synthetic(ng, 3, preset="cuda", device=dev, seed=mseed)
    geo = scene.geometry(dev, "cuda")
    mu, sc, rot = m._mu.detach(), m._scaling.detach(), m._rotation.detach()
    perm = slab_order(mu, None, 8, 1, size=sc.max(1).values, centroid=wall_centroid(geo.wall))
    # pairs of albedo rho <= 0 have no weight and are never enumerated (the float64-free part: the oracle's albedo)
    from oracle import torch_ref as R
    Pm = R.Params(*(t.detach()[perm] for t in (m._mu, m._scaling, m._rotation, m._opacity, m._features_dc,
                                               m._features_rest)), int(m.active_sh_degree), requires_grad=False)
    live = lambda p: R.albedo(Pm, geo.wall[p].float(), preset="cuda")[:, 0].numpy() > 0
    mu, sc, rot = (t[perm].double().numpy() for t in (mu, sc, rot))
    rng = np.random.default_rng(a.seed)
    small = a.scene == "small"
    nsp = fwd_nsplit(ng, geo.nwall)
    nw = a.walls or (geo.nwall if small else 4)
    walls = range(geo.nwall) if nw >= geo.nwall else sorted(rng.choice(geo.nwall, nw, replace=False).tolist())
    allw = [(s, w) for s in range(nsp) for w in range(4)]
    k = a.waves or (len(allw) if small else 3)
    waves = allw if k >= len(allw) else [allw[x] for x in sorted(rng.choice(len(allw), k, replace=False).tolist())]
    tot = replay_scene(geo, mu, sc, rot, walls=walls, waves=waves, max_chunks=a.chunks or (None if small else 6),
                       rule=a.rule, refill=a.refill, steps=a.steps, lw=a.lw, live=live)
    r = max(tot["rounds"], 1)
    print(json.dumps({"scene": a.scene, "rule": a.rule, "refill_at": a.refill, "steps": a.steps,
                      "wall_points": len(walls), "waves_per_wall_point": len(waves),
                      **{c: tot[c] for c in COUNTERS}, "entries_enumerated": tot["enumerated"],
                      "entries_requeued": tot["requeued"], "entries_per_refill": tot["entries_taken"] / max(tot["refills"], 1),
                      "refills_per_round": tot["refills"] / r, "active_per_round": tot["active_lane_rounds"] / r}))


if __name__ == "__main__":
    main()
