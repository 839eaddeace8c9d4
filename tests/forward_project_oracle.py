"""Float64 numpy restatement of the forward projection (include/nlosgr.h, ABI 13), fed the same fp32 inputs the
kernel reads, including the fp32 r0 and inv_dr.  For voxel centre x (grid tables) and wall point i:

    d = sqrt(dx*dx + dy*dy + dz*dz),  u = (d - r0) * inv_dr,  k = floor(u),  f = u - k
    rows_i[j] = sum_x d^power vol(x) ((1-f) [k == j] + f [k+1 == j]),   0 <= j < nr

(the scatter form of backproject_oracle.backproject64: the same coefficients, so the two are adjoint) and the
per-bin bound the GPU tests hold the kernel to, with no further factor:

    B_i[j] = sum_x |d^p vol| [ du 1{|u - j| < 2} + 8 2^-24 L(u - j) ]  +  N_ij q / 2  +  2^-24 |rows_i[j]|

    du = 6 2^-24 (d + |r0|) inv_dr   the fp32 error of u (three subtractions, the sum of squares, the sqrt and the
                                     scale); the splat L(u - j) = max(0, 1 - |u - j|) is 1-Lipschitz in u, so a
                                     different floor on the GPU is covered; it can move a voxel's share only in
                                     the bins within two of u
    8                                the roundings of the fp32 term (weight, product, 1 - f)
    N_ij q / 2                       each term is rounded once to the nearest multiple of the quantum q (quantum()
                                     restates the header's formula); N_ij counts the voxels with |u - j| < 2
    2^-24 |rows|                     the conversion of the bin's sum to fp32

The bound is derived, not tuned.
"""
import math

import numpy as np

import backproject_oracle as BO

U = BO.U
WEIGHT_MARGIN = 1.0 + 2.0 ** -19


def weight_bound(r0, inv_dr, power, nr):
    """wmax of the header: R^|power| by |power| multiplications from 1.0 (its reciprocal for power < 0) times
    1 + 2^-19, R = max(r0 + (nr + 1) dr, 0) or r0 - 1.5 dr, from the fp32 r0 and inv_dr in double."""
    r0, dr = float(np.float32(r0)), 1.0 / float(np.float32(inv_dr))
    R = r0 - 1.5 * dr if power < 0 else r0 + float(nr + 1) * dr
    R = max(R, 0.0)
    w = 1.0
    for _ in range(abs(int(power))):
        w *= R
    if power < 0:
        w = 1.0 / w
    return w * WEIGHT_MARGIN


def quantum(vmax, r0, inv_dr, power, nr, nvox):
    """q = 2^(e - S): S = 62 - ceil(log2(2 nvox)), e = ev + ew from frexp of max|vol| (fp32) and of wmax."""
    S = 62 - int(math.ceil(math.log2(2 * int(nvox))))
    assert 2 ** (62 - S) >= 2 * nvox > 2 ** (61 - S)
    ev = math.frexp(float(np.float32(vmax)))[1]
    ew = math.frexp(weight_bound(r0, inv_dr, power, nr))[1]
    return math.ldexp(1.0, ev + ew - S)


def _scatter(idx, ok, weights, nw, nr):
    """sum of weights[x, i] into [i, idx[x, i]] over the pairs where ok."""
    col = np.broadcast_to(np.arange(nw)[None, :], idx.shape)
    flat = (col[ok] * nr + idx[ok]).astype(np.int64)
    return np.bincount(flat, weights=weights[ok], minlength=nw * nr).reshape(nw, nr)


def forward64(vol, walls, xs, ys, zs, r0, inv_dr, nr, power, d=None, want_bound=True):
    """(rows [nwall, nr] float64, B [nwall, nr] float64 or None).  vol [nx, ny, nz]: the fp32 volume the kernel
    reads, or a float64 volume taken as it is (then the quantum is formed from its fp32-rounded maximum).  Any
    non-finite voxel: every row NaN, as the kernel documents.  d: distances64 of the same walls and tables."""
    v = np.asarray(vol).astype(np.float64).reshape(-1)
    nw = np.asarray(walls).reshape(-1, 3).shape[0]
    nr = int(nr)
    if nw == 0:
        z = np.zeros((0, nr))
        return z, (z.copy() if want_bound else None)
    if not np.isfinite(v).all():
        n = np.full((nw, nr), np.nan)
        return n, (n.copy() if want_bound else None)
    if d is None:
        d = BO.distances64(walls, xs, ys, zs)
    u = BO.bin_coordinate(d, r0, inv_dr)
    k = np.floor(u)
    f = u - k
    kc = np.clip(k, -4, nr + 2).astype(np.int64)        # beyond, no bin of the row is within two of u
    with np.errstate(divide="ignore", invalid="ignore"):
        wv = d ** int(power) * v[:, None]                # (a pair with d = 0 and power < 0 lies outside every mask)
    in0, in1 = (kc >= 0) & (kc < nr), (kc + 1 >= 0) & (kc + 1 < nr)
    rows = _scatter(kc, in0, (1.0 - f) * wv, nw, nr) + _scatter(kc + 1, in1, f * wv, nw, nr)
    if not want_bound:
        return rows, None
    a = np.abs(wv)
    du = 6.0 * U * (d + abs(float(np.float32(r0)))) * float(np.float32(inv_dr))
    one = np.ones_like(a)
    B = 8.0 * U * (_scatter(kc, in0, (1.0 - f) * a, nw, nr) + _scatter(kc + 1, in1, f * a, nw, nr))
    N = np.zeros((nw, nr))
    for off in (-1, 0, 1, 2):                           # |u - j| < 2: j = k - 1, k, k + 1, and k + 2 when f > 0
        j = kc + off
        ok = (j >= 0) & (j < nr) & ((f > 0) if off == 2 else True)
        B += _scatter(j, ok, du * a, nw, nr)
        N += _scatter(j, ok, one, nw, nr)
    vmax = float(np.abs(v.astype(np.float32)).max()) if v.size else 0.0
    if vmax > 0:
        B += N * (0.5 * quantum(vmax, r0, inv_dr, power, nr, v.size))
    B += U * np.abs(rows)
    return rows, B


def landweber64(rows, walls, tabs, r0, inv_dr, iterations=30, power_iterations=8):
    """(volume, objective [iterations + 1], eigenvalue): the projected gradient v <- max(v - A^T (A v - h) / L, 0)
    from zero in float64 (power 0), L the largest eigenvalue of A^T A after `power_iterations` power iterations
    from the all-ones volume; objective[n] = 1/2 |A v - h|^2 before update n, and the last entry after the last."""
    d = BO.distances64(walls, *tabs)
    shape = tuple(len(t) for t in tabs)
    nr = rows.shape[1]
    A = lambda v: forward64(v, walls, *tabs, r0, inv_dr, nr, 0, d=d, want_bound=False)[0]
    At = lambda h: BO.backproject64(h, walls, *tabs, r0, inv_dr, 0, d=d, want_bound=False)[0]
    v = np.ones(shape)
    for _ in range(power_iterations):
        v = At(A(v / np.linalg.norm(v)))
        lam = float(np.linalg.norm(v))
    h = np.asarray(rows).astype(np.float64)
    x = np.zeros(shape)
    obj = []
    for _ in range(iterations):
        res = A(x) - h
        obj.append(0.5 * float((res ** 2).sum()))
        x = np.maximum(x - At(res) / lam, 0.0)
    obj.append(0.5 * float(((A(x) - h) ** 2).sum()))
    return x, np.array(obj), lam


def shell_integral(r, D, s):
    """Integral over the sphere of radius r (centred at distance D from the Gaussian's mean) of an isotropic
    normalised-to-peak-1 Gaussian exp(-|x - mu|^2 / 2 s^2): 2 pi r s^2 / D (e^{-(r-D)^2 / 2 s^2} - e^{-(r+D)^2 / 2 s^2})."""
    return 2.0 * np.pi * r * s * s / D * (np.exp(-(r - D) ** 2 / (2 * s * s)) - np.exp(-(r + D) ** 2 / (2 * s * s)))
