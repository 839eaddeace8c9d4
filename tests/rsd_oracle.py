"""Float64 numpy restatement of the fast phasor field (include/nlosgr.h, the nlosgr_rsd_* symbols; nlosgr/rsd.py), fed
the same fp32 inputs the kernels get: the fp32 rows, tables, r0, dr, sx, sz, the laser spot and the complex64 band
coefficients.  Each stage is callable alone, and reconstruct64 is the independent reference for the whole: the direct
sum over wall points and band frequencies, with no FFT and no padded array at all.

    band     P = wavelength / (2 dr), sigma_b = cycles P / 6, theta_q = 2 pi q / Nt, theta_0 = 2 pi / P,
             q in [max(1, ceil(Nt/P - 3 sigma_q)), min(Nt/2 - 1, floor(Nt/P + 3 sigma_q))], sigma_q = Nt / (2 pi sigma_b)
             coef[q] = exp(-(sigma_b (theta_q - theta_0))^2 / 2) exp(-i theta_q r0 / dr) / Nt
    load     Pw[q - q_lo, m, n] = coef[q] S[row(m, n), q] at [0:H, 0:W] of a zero [nq, 2H, 2W], S = rfft(rows, Nt)
    kernel   K[j, q, a, b] = d^e exp(2 pi i frac(g q (d / dr) / Nt)), d = sqrt((a' sz)^2 + (b' sx)^2 + (ys[j] - y0)^2) over
             the signed offsets a', b'; 0 at a' = -H or b' = -W; (e, g) = (power, 1), with a laser (power / 2, 1/2)
    apply    Kf[j, q] Pf[q]
    gather   Phi[n, j, m] = sum_q L_q o[j, q, m, n]; L_q = 1, with a laser dl^(power/2) exp(2 pi i frac(q (dl/dr) / (2 Nt)))

Voxel (n, j, m) is the point (xs[n], ys[j], zs[m]); lattice point (m, n) is measured at (xs[n], y0, zs[m]).
"""
import math

import numpy as np

import backproject_oracle as BO
import fk_oracle as FO
import nonconfocal_oracle as NO

f32 = FO.f32


def _t64(t):
    return np.asarray(t, dtype=np.float32).astype(np.float64).reshape(-1)


def band64(wavelength, dr, Nt, r0, cycles=4.0):
    """(q_lo, coef complex128 [nq]) from the fp32 r0 and dr."""
    dr, r0 = f32(dr), f32(r0)
    P = float(wavelength) / (2.0 * dr)
    sb = float(cycles) * P / 6.0
    sq = Nt / (2.0 * math.pi * sb)
    q_lo = max(1, math.ceil(Nt / P - 3.0 * sq))
    q_hi = min(Nt // 2 - 1, math.floor(Nt / P + 3.0 * sq))
    q = np.arange(q_lo, q_hi + 1)
    th = 2.0 * np.pi * q / Nt
    return q_lo, np.exp(-0.5 * (sb * (th - 2.0 * np.pi / P)) ** 2) * np.exp(-1j * th * r0 / dr) / Nt


def c64(coef):
    """The coefficients as the complex64 values the kernels get, in complex128."""
    return np.asarray(coef).astype(np.complex64).astype(np.complex128)


def load64(S, H, W, q_lo, coef, perm=None, x_along="n"):
    """Pw [nq, 2H, 2W] complex128 from the spectrum S [H W, Nt/2 + 1] (taken to complex128 as it is)."""
    S = np.asarray(S).astype(np.complex128)
    coef = c64(coef)
    nq = len(coef)
    Pw = np.zeros((nq, 2 * H, 2 * W), dtype=np.complex128)
    band = S[FO.lattice_rows(H, W, perm, x_along)][:, :, q_lo:q_lo + nq]          # [H, W, nq]
    Pw[:, :H, :W] = (band * coef[None, None, :]).transpose(2, 0, 1)
    return Pw


def _pow_half(d, halves):
    return d ** (0.5 * halves)


def kernel64(ys, y0, H, W, sx, sz, dr, Nt, q_lo, nq, power=0, laser=False):
    """K [ny, nq, 2H, 2W] complex128."""
    D = _t64(ys) - f32(y0)
    sx, sz, dr = f32(sx), f32(sz), f32(dr)
    a, b = FO.signed(2 * H), FO.signed(2 * W)
    d = np.sqrt((a[None, :, None] * sz) ** 2 + (b[None, None, :] * sx) ** 2 + D[:, None, None] ** 2)   # [ny, 2H, 2W]
    g, halves = (0.5, int(power)) if laser else (1.0, 2 * int(power))
    q = np.arange(q_lo, q_lo + nq)
    turns = g * q[None, :, None, None] * (d[:, None] / dr) / Nt
    K = _pow_half(d, halves)[:, None] * np.exp(2j * np.pi * (turns - np.floor(turns)))
    zero = (a[:, None] == -H) | (b[None, :] == -W)
    return np.where(zero[None, None], 0.0, K)


def apply64(Kf, Pf):
    return np.asarray(Kf).astype(np.complex128) * np.asarray(Pf).astype(np.complex128)[None]


def gather64(o, H, W, q_lo, Nt, dr, xs, ys, zs, power=0, laser=None):
    """Phi [W, ny, H] complex128 from o [ny, nq, 2H, 2W] (its [0:H, 0:W] corner alone is read)."""
    o = np.asarray(o)[:, :, :H, :W].astype(np.complex128)
    nq = o.shape[1]
    if laser is None:
        return np.ascontiguousarray(o.sum(axis=1).transpose(2, 0, 1))
    xs, ys, zs, l, dr = _t64(xs), _t64(ys), _t64(zs), _t64(laser), f32(dr)
    dl = np.sqrt((xs[None, None, :] - l[0]) ** 2 + (ys[:, None, None] - l[1]) ** 2 + (zs[None, :, None] - l[2]) ** 2)
    q = np.arange(q_lo, q_lo + nq)
    turns = q[None, :, None, None] * (dl[:, None] / dr) / (2.0 * Nt)
    L = np.exp(2j * np.pi * (turns - np.floor(turns)))
    return np.ascontiguousarray((_pow_half(dl, int(power)) * (L * o).sum(axis=1)).transpose(2, 0, 1))


def staged64(rows, H, W, xs, zs, y0, ys, r0, dr, wavelength, Nt, cycles=4.0, power=0, laser=None, perm=None,
             x_along="n"):
    """Phi [W, ny, H] complex128 through the stages, with numpy's FFTs between them."""
    rows = np.asarray(rows, dtype=np.float32).astype(np.float64)
    sx, sz = spacings(xs, zs)
    q_lo, coef = band64(wavelength, dr, Nt, r0, cycles)
    Pf = np.fft.fft2(load64(np.fft.rfft(rows, n=Nt, axis=1), H, W, q_lo, coef, perm, x_along))
    K = kernel64(ys, y0, H, W, sx, sz, dr, Nt, q_lo, len(coef), power, laser is not None)
    o = np.fft.ifft2(apply64(np.fft.fft2(K), Pf))
    return gather64(o, H, W, q_lo, Nt, dr, xs, ys, zs, power, laser)


def spacings(xs, zs):
    """(sx, sz) as nlosgr.rsd forms them: float64 from the tables' end points, one point taking the other's."""
    xs, zs = _t64(xs), _t64(zs)
    sx = (xs[-1] - xs[0]) / (len(xs) - 1) if len(xs) > 1 else None
    sz = (zs[-1] - zs[0]) / (len(zs) - 1) if len(zs) > 1 else sx
    return (sz if sx is None else sx), sz


def _paths(H, W, xs, zs, y0, ys, laser):
    """(us [V, P], ul [V] or None, voxel shape): the sensor distances of every voxel (n, j, m) to every lattice point
    p = m' W + n' on the IDEAL lattice the kernels use (offsets times the spacing), and the laser distances."""
    xs, ys, zs = _t64(xs), _t64(ys), _t64(zs)
    sx, sz = spacings(xs, zs)
    sx, sz = f32(sx), f32(sz)
    n, j, m = np.meshgrid(np.arange(W), np.arange(len(ys)), np.arange(H), indexing="ij")
    n, j, m = n.reshape(-1), j.reshape(-1), m.reshape(-1)
    mp, np_ = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mp, np_ = mp.reshape(-1), np_.reshape(-1)
    D = ys[j] - f32(y0)
    us = np.sqrt(((m[:, None] - mp[None]) * sz) ** 2 + ((n[:, None] - np_[None]) * sx) ** 2 + D[:, None] ** 2)
    ul = None
    if laser is not None:
        l = _t64(laser)
        ul = np.sqrt((xs[n] - l[0]) ** 2 + (ys[j] - l[1]) ** 2 + (zs[m] - l[2]) ** 2)
    return us, ul, (W, len(ys), H)


def reconstruct64(rows, H, W, xs, zs, y0, ys, r0, dr, wavelength, Nt, cycles=4.0, power=0, laser=None):
    """Phi [W, ny, H] complex128: the direct sum  sum_p sum_q coef[q] S_p[q] w(x, p) exp(2 pi i q (u(x, p) / dr) / Nt)
    with S_p[q] the float64 DFT of row p = m W + n, u the half path and w the weight of backproject(..., lasers=)."""
    rows = np.asarray(rows, dtype=np.float32).astype(np.float64)
    drf = f32(dr)
    q_lo, coef = band64(wavelength, dr, Nt, r0, cycles)
    coef = c64(coef)
    q = np.arange(q_lo, q_lo + len(coef))
    jj = np.arange(rows.shape[1])
    T = coef[:, None] * (np.exp(-2j * np.pi * q[:, None] * jj[None, :] / Nt) @ rows.T)          # [nq, P]
    us, ul, shape = _paths(H, W, xs, zs, y0, ys, laser)
    if ul is None:
        u, w = us, us ** int(power)
    else:
        u, w = 0.5 * (us + ul[:, None]), (us * ul[:, None]) ** (0.5 * int(power))
    phi = np.zeros(us.shape[0], dtype=np.complex128)
    for i, qq in enumerate(q):
        phi += (w * np.exp(2j * np.pi * qq * (u / drf) / Nt)) @ T[i]
    return phi.reshape(shape)


def timedomain64(rows, H, W, xs, zs, y0, ys, r0, dr, wavelength, Nt, cycles=4.0, power=0, laser=None):
    """Phi [W, ny, H] complex128 with no band at all: every row filtered in time with the untruncated Morlet wavelet
    psi(s) = exp(-s^2 / (2 sigma_b^2)) / (sigma_b sqrt(2 pi)) exp(2 pi i s / P), evaluated at the continuous bin
    coordinate t = (u - r0) / dr and periodic in Nt, weighted as nonconfocal_oracle.weight64 / backproject_oracle."""
    rows = np.asarray(rows, dtype=np.float32).astype(np.float64)
    drf, r0f = f32(dr), f32(r0)
    P = float(wavelength) / (2.0 * drf)
    sb = float(cycles) * P / 6.0
    us, ul, shape = _paths(H, W, xs, zs, y0, ys, laser)
    if ul is None:
        u, w = us, us ** int(power)
    else:
        ulb = np.broadcast_to(ul[:, None], us.shape)
        u, w = 0.5 * (us + ulb), NO.weight64(us, ulb, power)
    t = (u - r0f) / drf                                                       # [V, P]
    phi = np.zeros(us.shape[0], dtype=np.complex128)
    for j in range(rows.shape[1]):
        s = t - j
        s = s - Nt * np.round(s / Nt)                                         # the nearest periodic image
        acc = np.zeros_like(t, dtype=np.complex128)
        for k in (-1, 0, 1):
            sk = s + k * Nt
            acc += np.exp(-sk * sk / (2.0 * sb * sb)) * np.exp(2j * np.pi * sk / P)
        phi += ((w * acc) * rows[None, :, j]).sum(axis=1)
    return (phi / (sb * math.sqrt(2.0 * math.pi))).reshape(shape)


# ---- the dense cases: lattice, window, DFT length, wavelength (P bins per period), depth planes, laser spot ---------

DENSE = {
    "8x8x32": dict(H=8, W=8, nr=32, sx=0.1, sz=0.1, dr=0.02, r0_bins=0, Nt=64, P=8.0, y0=0.0,
                   ys=(0.3, 0.37, 0.5, 0.52), laser=(0.137, 0.0, -0.083)),
    "5x7x17_r3": dict(FO.DENSE["5x7x17_r3"], Nt=40, P=6.0, y0=0.1, ys=(0.35, 0.5, 0.55), laser=(-0.211, 0.1, 0.067)),
    "12x20x48": dict(FO.DENSE["12x20x48"], Nt=96, P=8.0, y0=0.0, ys=(0.28, 0.4, 0.46, 0.6, 0.61), laser=(0.31, 0.0, 0.123)),
    "1x9x16": dict(FO.DENSE["1x9x16"], Nt=32, P=4.0, y0=0.0, ys=(0.2, 0.33), laser=(0.07, 0.0, 0.045)),
}


def dense_problem(name):
    """The keyword arguments of reconstruct64 / staged64 (but power and laser) of a dense case, and its laser spot."""
    c = DENSE[name]
    xs, zs, _ = FO.lattice(c["H"], c["W"], c["sx"], c["sz"])
    r0, dr = FO.window(c)
    kw = dict(rows=FO.dense_rows(c), H=c["H"], W=c["W"], xs=xs, zs=zs, y0=c["y0"],
              ys=np.asarray(c["ys"], dtype=np.float32), r0=r0, dr=dr, wavelength=c["P"] * 2.0 * dr, Nt=c["Nt"])
    return kw, np.asarray(c["laser"], dtype=np.float32)


# ---- point scatterers on the f-k tests' lattices --------------------------------------------------------------

SCATTERER_LASER = (0.11, 0.0, -0.07)       # off the lattice, off the wall's centre
SCATTERER_SPAN = 6                          # depth planes on either side of the scatterer's bin
# wavelength in units of the wall spacing sx (2 to 4), per lattice: test_rsd_cpu asserts the oracle's peak for each
SCATTERER_WAVELENGTH = {"16x16x64": 3.0, "12x20x48": 3.0, "16x16x64_r20": 3.0, "16x16x64_r35": 3.0}


def scatterer_problem(name, with_laser):
    """(kw, laser, voxel): the keyword arguments (but Nt, power, laser) of one point scatterer of FO.SCATTERERS seen by
    its lattice (the linear splat of backproject_oracle / nonconfocal_oracle.scatterer_rows, unweighted), depth
    planes at the bins' depths around it, and the scatterer's voxel (n, j, m) in that volume."""
    c = FO.SCATTERERS[name]
    xs, zs, walls = FO.lattice(c["H"], c["W"], c["sx"], c["sz"])
    dr = f32(c["dr"])
    r0 = f32(c["r0_bins"] * c["dr"])
    n, j, m = c["voxel"]
    inv_dr = float(np.float32(1.0) / np.float32(dr))
    bins = np.arange(max(j - SCATTERER_SPAN, 1 if c["r0_bins"] == 0 else 0), min(j + SCATTERER_SPAN, c["nr"] - 1) + 1)
    ys = (r0 + bins * dr).astype(np.float32)
    point = np.array([xs[n], ys[int(np.nonzero(bins == j)[0][0])], zs[m]], dtype=np.float32)
    laser = np.asarray(SCATTERER_LASER, dtype=np.float32) if with_laser else None
    if with_laser:
        rows, _ = NO.scatterer_rows(walls, laser[None], point, r0, inv_dr, c["nr"])
    else:
        rows = BO.scatterer_rows(walls, point, r0, inv_dr, c["nr"])
    kw = dict(rows=rows, H=c["H"], W=c["W"], xs=xs, zs=zs, y0=0.0, ys=ys, r0=r0, dr=dr,
              wavelength=SCATTERER_WAVELENGTH[name] * c["sx"])
    return kw, laser, (n, int(np.nonzero(bins == j)[0][0]), m)


def argmax3(vol):
    return tuple(int(v) for v in np.unravel_index(int(np.argmax(np.asarray(vol))), np.asarray(vol).shape))
