"""Float64 numpy restatements of the non-confocal back-projection and forward projection (include/nlosgr.h,
nlosgr_backproject_nc / nlosgr_forward_project_nc), fed the same fp32 inputs the kernels read, including the
fp32 r0, inv_dr and dmin.  For voxel centre x, sensed point s_i and laser spot l_i:

    ds = |x - s_i|, dl = |x - l_i|,  g = (dl + ds) / 2,  m = dl ds
    u = (g - r0) * inv_dr,  k = floor(u),  f = u - k,  weight = m^(power/2)
    out(x)    = sum_i weight ((1-f) h_i[k] + f h_i[k+1])                       h_i[j] = 0 outside [0, nr)
    rows_i[j] = sum_x weight vol(x) ((1-f) [k == j] + f [k+1 == j])            pairs with min(dl, ds) < dmin left
                                                                               out when power < 0

The bounds are the confocal ones (backproject_oracle.py, forward_project_oracle.py) with the roundings the
non-confocal arithmetic adds, derived and not tuned on GPU output:

    back-projection   B(x) = sum_i weight [ du_i S_i + 266 2^-24 (|h_i[k]| + |h_i[k+1]|) ]
    forward           B_i[j] = sum_x |weight vol| [ du 1{|u - j| < 2} + 10 2^-24 L(u - j) ] + N_ij q / 2
                               + 2^-24 |rows_i[j]|

    du = 7 2^-24 (g + |r0|) inv_dr   the confocal 6 (per distance: three subtractions, the sum of squares, the
                                     sqrt; then the scale) plus the one rounding of dl + ds.  Each distance's error
                                     enters g with weight 1/2, so the two distances together cost what the
                                     confocal d costs; the halving is exact
    266 = 264 + 2, 10 = 8 + 2        the weight gains two roundings over the confocal d^p: the product m = dl ds
                                     of two separately rounded distances, and sqrt(m) for the odd powers
    S_i, the mask -2 <= k <= nr, L, N_ij, q: as in the confocal oracles; q is formed with wmax from R = dmin for
    a negative power (quantum()).

An fp32 numpy emulation of the back-projection kernel's arithmetic (emulate32) stays at <= 0.012 B on the
test grid, while a shifted bin, another power and the confocal operator on the same inputs are each more than
100 B away somewhere (test_nonconfocal_cpu.py).
"""
import math

import numpy as np

import backproject_oracle as BO
import forward_project_oracle as FO

U = BO.U
PAD = BO.PAD


def _points(p):
    return np.asarray(p, dtype=np.float32).astype(np.float64).reshape(-1, 3)


def distances64(sensors, lasers, xs, ys, zs):
    """(ds, dl): [V, nmeas] float64 distances of every voxel centre to every sensed point and to every
    measurement's laser spot (lasers [nmeas, 3] or [1, 3])."""
    ds = BO.distances64(sensors, xs, ys, zs)
    dl = BO.distances64(lasers, xs, ys, zs)
    return ds, np.broadcast_to(dl, ds.shape) if dl.shape[1] == 1 else dl


def weight64(ds, dl, power):
    """m^(power/2), m = dl ds (inf where m = 0 and power < 0)."""
    with np.errstate(divide="ignore"):
        return (dl * ds) ** (0.5 * int(power))


def bin_coordinate(ds, dl, r0, inv_dr):
    return BO.bin_coordinate(0.5 * (dl + ds), r0, inv_dr)


def _du(ds, dl, r0, inv_dr):
    return 7.0 * U * (0.5 * (dl + ds) + abs(float(np.float32(r0)))) * float(np.float32(inv_dr))


def backproject64(rows, sensors, lasers, xs, ys, zs, r0, inv_dr, power, d=None, want_bound=True):
    """(out [nx,ny,nz] float64, B [nx,ny,nz] float64 or None).  d: distances64 of the same points and tables."""
    rows = np.asarray(rows)
    nw, nr = rows.shape
    shape = (len(xs), len(ys), len(zs))
    if nw == 0:
        z = np.zeros(shape)
        return z, (z.copy() if want_bound else None)
    ds, dl = distances64(sensors, lasers, xs, ys, zs) if d is None else d
    u = bin_coordinate(ds, dl, r0, inv_dr)
    k = np.floor(u)
    f = u - k
    kc = np.clip(k, -3, nr + 1).astype(np.int64)       # outside [-2, nr] every bin around k is a padding zero
    hp = np.zeros((nw, nr + 2 * PAD))
    hp[:, PAD:PAD + nr] = rows.astype(np.float64)
    idx = kc + PAD
    col = np.arange(nw)[None, :]
    h0, h1 = hp[col, idx], hp[col, idx + 1]
    w = weight64(ds, dl, power)
    with np.errstate(invalid="ignore"):
        out = (w * ((1.0 - f) * h0 + f * h1)).sum(axis=1)
        if not want_bound:
            return out.reshape(shape), None
        hm, h2 = hp[col, idx - 1], hp[col, idx + 2]
        S = np.maximum(np.maximum(np.abs(h0 - hm), np.abs(h1 - h0)), np.abs(h2 - h1))
        term = _du(ds, dl, r0, inv_dr) * S + 266.0 * U * (np.abs(h0) + np.abs(h1))
        term = np.where((k >= -2) & (k <= nr), term, 0.0)
        B = (w * term).sum(axis=1)
    return out.reshape(shape), B.reshape(shape)


def emulate32(rows, sensors, lasers, xs, ys, zs, r0, inv_dr, power, tile=256):
    """The back-projection kernel's arithmetic in numpy fp32 (every operation rounded to fp32, the distances in
    the kernel's order, the correctly rounded sqrt in place of the hardware's 1-ulp one, no fma), the tile sums
    in fp32 term by term and the tiles in float64."""
    f32 = np.float32
    rows = np.asarray(rows, dtype=f32)
    nw, nr = rows.shape
    g = np.meshgrid(*(np.asarray(t, dtype=f32) for t in (xs, ys, zs)), indexing="ij")
    X = np.stack(g, axis=-1).reshape(-1, 3)
    Ws = np.asarray(sensors, dtype=f32).reshape(-1, 3)
    Wl = np.asarray(lasers, dtype=f32).reshape(-1, 3)
    r0, inv_dr = f32(r0), f32(inv_dr)
    acc = np.zeros(X.shape[0], dtype=np.float64)
    hp = np.zeros((nw, nr + 2 * PAD), dtype=f32)
    hp[:, PAD:PAD + nr] = rows

    def dist(p):
        dx, dy, dz = X[:, 0] - p[0], X[:, 1] - p[1], X[:, 2] - p[2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz)

    for base in range(0, nw, tile):
        s = np.zeros(X.shape[0], dtype=f32)
        for i in range(base, min(nw, base + tile)):
            ds, dl = dist(Ws[i]), dist(Wl[i if Wl.shape[0] > 1 else 0])
            gh = f32(0.5) * (dl + ds)
            m = dl * ds
            u = np.minimum(np.maximum((gh - r0) * inv_dr, f32(-2.0)), f32(nr + 1))
            kf = np.floor(u)
            f = u - kf
            k = kf.astype(np.int64) + PAD
            h0, h1 = hp[i, k], hp[i, k + 1]
            sv = (f32(1.0) - f) * h0 + f * h1
            w = [np.ones_like(m), np.sqrt(m), m, m * np.sqrt(m), m * m][int(power)]
            s = s + w * sv
        acc += s.astype(np.float64)
    return acc.astype(f32).reshape(len(xs), len(ys), len(zs))


def weight_bound(r0, inv_dr, power, nr, dmin=None):
    """wmax of the header: the confocal one (forward_project_oracle.weight_bound) with R = dmin (fp32) for a
    negative power."""
    if power >= 0:
        return FO.weight_bound(r0, inv_dr, power, nr)
    w = 1.0
    for _ in range(-int(power)):
        w *= float(np.float32(dmin))
    return (1.0 / w) * FO.WEIGHT_MARGIN


def quantum(vmax, r0, inv_dr, power, nr, nvox, dmin=None):
    """q = 2^(e - S) as forward_project_oracle.quantum, with this module's weight_bound."""
    S = 62 - int(math.ceil(math.log2(2 * int(nvox))))
    ev = math.frexp(float(np.float32(vmax)))[1]
    ew = math.frexp(weight_bound(r0, inv_dr, power, nr, dmin))[1]
    return math.ldexp(1.0, ev + ew - S)


def forward64(vol, sensors, lasers, xs, ys, zs, r0, inv_dr, nr, power, dmin=None, d=None, want_bound=True):
    """(rows [nmeas, nr] float64, B [nmeas, nr] float64 or None).  dmin (power < 0): the fp32 value the kernel
    gets; pairs with min(dl, ds) < dmin are left out of the rows and of the bound."""
    v = np.asarray(vol).astype(np.float64).reshape(-1)
    nw = np.asarray(sensors).reshape(-1, 3).shape[0]
    nr = int(nr)
    if nw == 0:
        z = np.zeros((0, nr))
        return z, (z.copy() if want_bound else None)
    if not np.isfinite(v).all():
        n = np.full((nw, nr), np.nan)
        return n, (n.copy() if want_bound else None)
    ds, dl = distances64(sensors, lasers, xs, ys, zs) if d is None else d
    u = bin_coordinate(ds, dl, r0, inv_dr)
    k = np.floor(u)
    f = u - k
    kc = np.clip(k, -4, nr + 2).astype(np.int64)        # beyond, no bin of the row is within two of u
    live = np.ones(ds.shape, dtype=bool)
    if power < 0:
        live = np.minimum(dl, ds) >= float(np.float32(dmin))
    with np.errstate(divide="ignore", invalid="ignore"):
        wv = np.where(live, weight64(ds, dl, power) * v[:, None], 0.0)
    in0, in1 = live & (kc >= 0) & (kc < nr), live & (kc + 1 >= 0) & (kc + 1 < nr)
    rows = FO._scatter(kc, in0, (1.0 - f) * wv, nw, nr) + FO._scatter(kc + 1, in1, f * wv, nw, nr)
    if not want_bound:
        return rows, None
    a = np.abs(wv)
    du = _du(ds, dl, r0, inv_dr)
    one = np.ones_like(a)
    B = 10.0 * U * (FO._scatter(kc, in0, (1.0 - f) * a, nw, nr) + FO._scatter(kc + 1, in1, f * a, nw, nr))
    N = np.zeros((nw, nr))
    for off in (-1, 0, 1, 2):                           # |u - j| < 2: j = k - 1, k, k + 1, and k + 2 when f > 0
        j = kc + off
        ok = live & (j >= 0) & (j < nr) & ((f > 0) if off == 2 else True)
        B += FO._scatter(j, ok, du * a, nw, nr)
        N += FO._scatter(j, ok, one, nw, nr)
    vmax = float(np.abs(v.astype(np.float32)).max()) if v.size else 0.0
    if vmax > 0:
        B += N * (0.5 * quantum(vmax, r0, inv_dr, power, nr, v.size, dmin))
    B += U * np.abs(rows)
    return rows, B


def scatterer_rows(sensors, lasers, point, r0, inv_dr, nr):
    """[nmeas, nr] fp32: every measurement's histogram of one point scatterer, the linear splat (1-f, f) at the
    non-confocal bin coordinate of the point (bins outside the window dropped)."""
    Ws, Wl = _points(sensors), _points(lasers)
    p = np.asarray(point, dtype=np.float32).astype(np.float64)
    ds = np.sqrt(((Ws - p[None]) ** 2).sum(axis=1))
    dl = np.broadcast_to(np.sqrt(((Wl - p[None]) ** 2).sum(axis=1)), ds.shape)
    u = bin_coordinate(ds, dl, r0, inv_dr)
    k = np.floor(u).astype(np.int64)
    f = u - k
    rows = np.zeros((Ws.shape[0], nr))
    for b, val in ((k, 1.0 - f), (k + 1, f)):
        ok = (b >= 0) & (b < nr)
        rows[np.nonzero(ok)[0], b[ok]] += val[ok]
    return rows.astype(np.float32), u


# the cases of the tests: the confocal tests' tables (the volume reaches in front of the window and behind it),
# sensed points and laser spots uniform in [-0.5, 0.5]^2 on the wall y = 0, sensed point 0 on voxel (0, 0, 0)
FAR = 0.9           # half-path of the window's end


def tables(shape):
    nx, ny, nz = shape
    return (np.linspace(-0.3, 0.3, nx).astype(np.float32), np.linspace(0.0, 0.6, ny).astype(np.float32),
            np.linspace(-0.3, 0.3, nz).astype(np.float32))


def wall_points(n, g):
    w = np.zeros((n, 3), dtype=np.float32)
    w[:, 0] = g.random(n) - 0.5
    w[:, 2] = g.random(n) - 0.5
    return w


def problem(shape, nmeas, nr, r0, seed=0):
    """dict(shape, nmeas, nr, r0, dr, tabs, sensors, lasers [nmeas, 3], rows [nmeas, nr], vol, d=(ds, dl))."""
    g = np.random.default_rng(seed + 1000 * nmeas + nr + sum(shape))
    tabs = tables(shape)
    sensors = wall_points(nmeas, g)
    sensors[0] = (tabs[0][0], tabs[1][0], tabs[2][0])
    lasers = wall_points(nmeas, g)
    rows = g.standard_normal((nmeas, nr)).astype(np.float32)
    vol = g.standard_normal(shape).astype(np.float32)
    return dict(shape=shape, nmeas=nmeas, nr=nr, r0=r0, dr=(FAR - r0) / nr, tabs=tabs, sensors=sensors, lasers=lasers,
                rows=rows, vol=vol, d=distances64(sensors, lasers, *tabs))


def window(c):
    """(r0, inv_dr) of a problem as the fp32 values the kernels get (nlosgr.backproject.fp32_window)."""
    return float(np.float32(c["r0"])), float(np.float32(1.0) / np.float32(c["dr"]))
