"""Float64 replay, on the CPU, of the forward's candidate enumeration (csrc/nlosgr_volume.hpp, csrc/nlosgr_volume_fwd.hip): the bounding-sphere
(theta, phi) box of pair_setup, the support of ray_setup (quadric test, [kl, kh]) and the way passing cells are
grouped into ray queue entries: today's parent scheme ("trip": row-major trips of 3 cells that wrap across rows,
two adjacent passing cells of a trip pair up) and the run-following scheme of enumerate_runs ("run": trips of 4
cells of one row, trip_plan of csrc/nlosgr_enum.hpp).  Used by scripts/twin_estimate.py and by
tests/test_gpu_fx_runs.py, which compares the kernel's group count with these counts.  cuda preset only.
"""
import math

import numpy as np

K_ANG_MARGIN = 1e-4
TRIP_CELLS = 4


def quat_rot(q):
    """[n, 4] (r, x, y, z), normalised here -> rotation matrices [n, 3, 3]."""
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def gaussian_frames(mu, log_scaling, rotation, mod=1.0):
    """(A [n, 3, 3] = diag(1 / s) R^T, s_max [n]) of the cuda preset (s = exp(S) mod + 1e-8)."""
    s = np.exp(np.asarray(log_scaling, np.float64)) * mod + 1e-8
    R = quat_rot(np.asarray(rotation, np.float64))
    A = np.transpose(R, (0, 2, 1)) / s[:, :, None]
    return A, s.max(1)


def wall_point_cells(geo, p, mu, A, smax, cutoff, details=False):
    """One wall point against every Gaussian.  Returns (box [n, 4] = i0, i1, j0, j1 inclusive, ok [n, nt, np] =
    the cell is inside the box, passes the quadric test and has bins, kl, kh [n, nt, np]).  details: a fifth
    value, a dict of [n, nt, np] arrays for scripts/refill_replay.py: "pass" = inside the box and passing the
    quadric test (what the enumeration queues, bins or not), "a" = |A d|^2, "ks" = the closest-approach bin,
    "m2" = the squared Mahalanobis distance at the closest approach, and "dr" = the bin width."""
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)
    st, ct = f(geo.sin_theta[p]), f(geo.cos_theta[p])
    cp, sp = f(geo.cos_phi[p]), f(geo.sin_phi[p])
    th0, dth, ph0, dph = f(geo.grid_lin[p])
    w = f(geo.wall[p])
    r = f(geo.r)
    nr, nt, np_ = len(r), len(st), len(cp)
    r0 = r[0]
    dr = (r[-1] - r[0]) / (nr - 1)
    # cutoff: one number, or one radius per Gaussian [n] (scripts/trim_estimate.py: the trimmed support of
    # NLOSGR_FLAG_FX_TRIM, which takes the pair's own radius in the box, the quadric and the bin range)
    cutoff = np.asarray(cutoff, np.float64)
    mc2 = cutoff * cutoff
    if mc2.ndim:
        mc2 = mc2[:, None, None]
    n = len(mu)
    # the box (pair_setup)
    d = mu - w
    Rb = cutoff * smax * 1.0001 + 1e-7
    rxy2 = d[:, 0] ** 2 + d[:, 1] ** 2
    dist2 = rxy2 + d[:, 2] ** 2
    box = np.tile(np.array([0, nt - 1, 0, np_ - 1]), (n, 1))
    out = dist2 > Rb * Rb
    rxy, dist = np.sqrt(rxy2), np.sqrt(dist2)
    alpha = np.arctan2(Rb, np.sqrt(np.maximum(dist2 - Rb * Rb, 0))) + K_ANG_MARGIN
    thc = np.arctan2(rxy, d[:, 2])
    if dth > 0:
        box[out, 0] = np.clip(np.ceil((thc - alpha - th0) / dth), 0, nt - 1)[out]
        box[out, 1] = np.clip(np.floor((thc + alpha - th0) / dth), -1, nt - 1)[out]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (Rb / dist) / (rxy / dist)
    nar = out & (thc - alpha > 1e-3) & (thc + alpha < math.pi - 1e-3) & (dph > 0) & (ratio < 0.999)
    dphi = np.arcsin(np.clip(np.where(nar, ratio, 0), 0, 1)) + K_ANG_MARGIN
    phc = np.arctan2(d[:, 1], d[:, 0])
    lo, hi = phc - dphi, phc + dphi
    nar &= (lo > -math.pi) & (hi < math.pi)
    if dph > 0:
        box[nar, 2] = np.clip(np.ceil((lo - ph0) / dph), 0, np_ - 1)[nar]
        box[nar, 3] = np.clip(np.floor((hi - ph0) / dph), -1, np_ - 1)[nar]
    # the support of every ray (ray_setup)
    D = np.stack([st[:, None] * cp[None, :], st[:, None] * sp[None, :], np.broadcast_to(ct[:, None], (nt, np_))], -1)
    u0 = np.einsum("nij,nj->ni", A, w - mu)
    V = np.einsum("nij,tpj->ntpi", A, D)
    av = (V * V).sum(-1)
    b = np.einsum("ntpi,ni->ntp", V, u0)
    ts = -b / av
    m2 = (u0 * u0).sum(-1)[:, None, None] - b * b / av
    ks = (ts - r0) / dr
    hk = np.sqrt(np.maximum(mc2 - m2, 0) / av) / dr
    kl = np.clip(np.ceil(ks - hk), 0, nr)
    kh = np.clip(np.floor(ks + hk), -1, nr - 1)
    ii = np.arange(nt)[None, :, None]
    jj = np.arange(np_)[None, None, :]
    inbox = ((ii >= box[:, 0, None, None]) & (ii <= box[:, 1, None, None]) &
             (jj >= box[:, 2, None, None]) & (jj <= box[:, 3, None, None]))
    ok = inbox & (m2 <= mc2) & (kl <= kh)
    if details:
        return box, ok, kl.astype(np.int64), kh.astype(np.int64), {"pass": inbox & (m2 <= mc2), "a": av, "ks": ks,
                                                                   "m2": m2, "dr": dr}
    return box, ok, kl.astype(np.int64), kh.astype(np.int64)


def trip_plan(bits, n, cont, K):
    """csrc/nlosgr_enum.hpp trip_plan: ([(start, length)], cells consumed)."""
    groups, u = [], 0
    while u < n:
        if not (bits >> u) & 1:
            u += 1
            continue
        l = 1
        while l < K and u + l < n and (bits >> (u + l)) & 1:
            l += 1
        if l < K and u + l == n and cont and u > 0:
            return groups, u
        groups.append((u, l))
        u += l
    return groups, n


def groups_trip(okb, nc=3):
    """Parent scheme on one box (okb [rows, cols] bool).  Returns ([(row, col, length)], cells tested, trips)."""
    nrow, ncol = okb.shape
    cells = [(i, j) for i in range(nrow) for j in range(ncol)]
    out = []
    for c0 in range(0, len(cells), nc):
        trip = cells[c0:c0 + nc]
        u = 0
        while u < len(trip):
            i, j = trip[u]
            if not okb[i, j]:
                u += 1
            elif u + 1 < len(trip) and trip[u + 1] == (i, j + 1) and okb[i, j + 1]:
                out.append((i, j, 2))
                u += 2
            else:
                out.append((i, j, 1))
                u += 1
    return out, len(cells), (len(cells) + nc - 1) // nc


def groups_run(okb, K):
    """Run-following scheme on one box.  Returns ([(row, col, length)], cells tested, trips)."""
    nrow, ncol = okb.shape
    out, tested, trips = [], 0, 0
    for i in range(nrow):
        row = okb[i]
        c = 0
        while c < ncol:
            n = min(TRIP_CELLS, ncol - c)
            bits = sum(1 << u for u in range(n) if row[c + u])
            gs, used = trip_plan(bits, n, ncol - c > TRIP_CELLS, K)
            out += [(i, c + s, l) for s, l in gs]
            tested += n
            trips += 1
            c += used
    return out, tested, trips


def row_optimum(okb, K=2):
    """The most rays any pairing within rows can put into groups of K: sum over runs of K floor(run / K)."""
    tot = 0
    for row in okb:
        run = 0
        for v in list(row) + [False]:
            if v:
                run += 1
            else:
                tot += K * (run // K)
                run = 0
    return tot


def lane_rounds(groups, kl, kh, steps):
    """Drain rounds of the queue entries (a round starts at the even bin at or below an entry's first bin)."""
    tot = 0
    for i, j, l in groups:
        lo = int(kl[i, j:j + l].min())
        hi = int(kh[i, j:j + l].max())
        tot += -(-(hi - lo + 1 + (lo & 1)) // steps)
    return tot
