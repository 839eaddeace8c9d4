"""Float64 numpy restatement of the phasor-field reconstruction (nlosgr/phasor.py, nlosgr_backproject_phasor):

    P = wavelength / (2 dr),  sigma_b = cycles P / 6,  n = ceil(3 sigma_b),  m = -n..n
    env[m] = exp(-m^2 / (2 sigma_b^2)) / sum,  cos taps env cos(2 pi m / P),  sin taps env sin(2 pi m / P)
    y_i = h_i * (cos taps) + i h_i * (sin taps)          centre n, h = 0 outside the row (irf_oracle.apply64)
    re(x), im(x) = the back-projection of each channel   backproject_oracle / nonconfocal_oracle .backproject64
    mag(x) = sqrt(re^2 + im^2)

Nothing new is bounded here: each plane is one real back-projection, so its float64 value and its per-voxel bound
B are the confocal or the non-confocal oracle's, fed that channel's rows.
"""
import math

import numpy as np

import backproject_oracle as BO
import irf_oracle as IO
import nonconfocal_oracle as NO


def kernel64(wavelength, dr, cycles=4.0):
    """(cos taps, sin taps, n) in float64."""
    P = float(wavelength) / (2.0 * float(dr))
    sigma = float(cycles) * P / 6.0
    n = int(math.ceil(3.0 * sigma))
    m = np.arange(-n, n + 1, dtype=np.float64)
    env = np.exp(-(m ** 2) / (2.0 * sigma ** 2))
    env = env / env.sum()
    return env * np.cos(2.0 * np.pi * m / P), env * np.sin(2.0 * np.pi * m / P), n


def rows64(rows, wavelength, dr, cycles=4.0, fp32_taps=True):
    """[nmeas, nr, 2] float64: the rows convolved with both wavelets.  fp32_taps: the taps rounded to fp32 first,
    as the library's IRF holds them."""
    c, s, n = kernel64(wavelength, dr, cycles)
    if fp32_taps:
        c, s = c.astype(np.float32).astype(np.float64), s.astype(np.float32).astype(np.float64)
    return np.stack((IO.apply64(rows, c, n, 0.0), IO.apply64(rows, s, n, 0.0)), axis=-1)


def backproject64(rows_c, walls, xs, ys, zs, r0, inv_dr, power, lasers=None, want_bound=True):
    """(planes [2, nx, ny, nz], B [2, nx, ny, nz] or None, mag [nx, ny, nz]) in float64 from complex rows
    [nmeas, nr, 2] (fp32 as the kernel reads them, or float64): each channel through the confocal oracle
    (lasers None) or the non-confocal one."""
    rows_c = np.asarray(rows_c)
    planes, bounds = [], []
    for ch in range(2):
        r = rows_c[..., ch]
        if lasers is None:
            out, B = BO.backproject64(r, walls, xs, ys, zs, r0, inv_dr, power, want_bound=want_bound)
        else:
            out, B = NO.backproject64(r, walls, lasers, xs, ys, zs, r0, inv_dr, power, want_bound=want_bound)
        planes.append(out)
        bounds.append(B)
    planes = np.stack(planes)
    with np.errstate(invalid="ignore"):
        mag = np.sqrt(planes[0] ** 2 + planes[1] ** 2)
    return planes, (np.stack(bounds) if want_bound else None), mag


def magnitude32(re, im):
    """float32(sqrt(float64(re)^2 + float64(im)^2)) of fp32 planes: what mag is defined as."""
    re, im = np.asarray(re, dtype=np.float32).astype(np.float64), np.asarray(im, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(re * re + im * im).astype(np.float32)


def peak(mag):
    """(argmax index tuple, peak / second-largest voxel)."""
    flat = np.asarray(mag, dtype=np.float64).reshape(-1)
    order = np.argsort(flat)
    return tuple(int(v) for v in np.unravel_index(order[-1], mag.shape)), float(flat[order[-1]] / flat[order[-2]])


# the displaced-laser variant of backproject_oracle.SCENE's point scatterer: laser i = sensed point i moved by
# LASER_SHIFT along the wall (test_phasor_cpu.py checks the oracle's argmax and margin for it)
LASER_SHIFT = (0.1, 0.0, 0.05)


def nc_scatterer_scene(shift=LASER_SHIFT):
    """(rows, sensors, lasers, tabs, r0, inv_dr) of SCENE's scatterer seen with displaced lasers."""
    S = BO.SCENE
    walls = BO.relay_wall(*S["wall"])
    lasers = (walls + np.asarray(shift, dtype=np.float32)[None]).astype(np.float32)
    tabs = BO.linspace_tables(S["position"], S["size"], S["res"])
    r0, inv_dr = BO.scene_window()
    i, j, k = S["voxel"]
    rows, _ = NO.scatterer_rows(walls, lasers, (tabs[0][i], tabs[1][j], tabs[2][k]), r0, inv_dr, S["nr"])
    return rows, walls, lasers, tabs, r0, inv_dr
