"""Float64 numpy restatement of the light-cone transform (include/nlosgr.h, the nlosgr_lct_* symbols), fed the same
fp32 inputs the kernels get: the fp32 rows and the fp32 r0, dr, sx, sz, snr.  Each stage is callable alone.  The
lattices and rows are those of tests/fk_oracle.py (DENSE, dense_rows, scatterer_scene, lattice, window).

Input: rows [H W, nr] as for f-k migration; nv depth-squared cells (default nr).  Nz = 2 H, Nx = 2 W, Nv = 2 nv.

    edges       bin j owns r in [e_j, e_j+1), e_j = r0 + (j - 1/2) dr, e_0 clamped at 0;  v_lo = e_0^2, v_hi = e_nr^2,
                dv = (v_hi - v_lo) / nv;  cell i owns r in [t_i, t_i+1), t_i = sqrt(v_lo + i dv), t_0 = e_0, t_nv = e_nr
    resampling  R[i, j] = |cell i n bin j| / (t_i+1 - t_i) / ((t_i + t_i+1) / 2)                          [nv, nr]
    load        psi[m, n, j] = max(rows[v, j], 0) (r0 + j dr)^power;  g = R psi along the last axis, at
                [0:H, 0:W, 0:nv] of a zero array [Nz, Nx, Nv]
    kernel      signed DFT indices c (z), b (x):  s = ((b sx)^2 + (c sz)^2) / dv, k = floor(s), f = s - k,
                K[c, b, k] = scale (1 - f) where k <= nv - 1, K[c, b, k + 1] = scale f where k + 1 <= nv - 1, zero
                elsewhere;  scale = 1 / ||K||_2
    inverse     Fk = fftn(K);  G = conj(Fk) / (|Fk|^2 + 1 / snr), or conj(Fk) with backprop
                o = ifftn(fftn(pad) G)
    store       volume[n, j, m] = max(sum_i R[i, j] Re o[m, n, i], 0):  [W, nr, H]

Voxel (n, j, m) is the point (xs[n], y0 + r0 + j dr, zs[m]).
"""
import numpy as np

import fk_oracle as FO


# the point-scatterer checks: (lattice of fk_oracle.SCATTERERS, nv, the scatterer's voxel or None for the lattice's own).
# On the r0 = 35 dr lattice the near voxel (6, 8, 9) needs nv = 128: at nv = 64 a near cell is two bins deep and the
# peak sits one bin early.
PEAKS = [("16x16x64", None, None), ("12x20x48", None, None), ("16x16x64_r20", None, None),
         ("16x16x64_r35", 64, (6, 30, 9)), ("16x16x64_r35", 128, None)]


def peak_case(name, voxel):
    """The scatterer lattice `name` with its scatterer moved to `voxel` (None: left where it is)."""
    c = dict(FO.SCATTERERS[name])
    if voxel is not None:
        c["voxel"] = voxel
    return c


def edges64(r0, dr, nr, nv=None):
    """(e [nr + 1], t [nv + 1], dv): the bin edges, the cell edges and the cell width in r^2."""
    r0, dr = FO.f32(r0), FO.f32(dr)
    nv = nr if nv is None else int(nv)
    e = r0 + (np.arange(nr + 1) - 0.5) * dr
    e[0] = max(e[0], 0.0)
    v_lo, v_hi = e[0] ** 2, e[nr] ** 2
    dv = (v_hi - v_lo) / nv
    t = np.sqrt(v_lo + np.arange(nv + 1) * dv)
    t[0], t[nv] = e[0], e[nr]
    return e, t, dv


def resampling64(r0, dr, nr, nv=None):
    """(R [nv, nr] float64 dense, dv)."""
    e, t, dv = edges64(r0, dr, nr, nv)
    overlap = np.minimum(t[1:, None], e[None, 1:]) - np.maximum(t[:-1, None], e[None, :-1])
    overlap = np.clip(overlap, 0.0, None)
    R = overlap / (t[1:] - t[:-1])[:, None] / ((t[:-1] + t[1:]) / 2)[:, None]
    return R, dv


def load64(rows, H, W, r0, dr, R, power=4, perm=None, x_along="n"):
    """The padded array [2H, 2W, 2nv], complex128 (imaginary part zero)."""
    rows = np.asarray(rows, dtype=np.float32).astype(np.float64)
    nv, nr = R.shape
    r = FO.f32(r0) + np.arange(nr) * FO.f32(dr)
    psi = np.maximum(rows[FO.lattice_rows(H, W, perm, x_along)], 0.0) * r[None, None, :] ** int(power)
    pad = np.zeros((2 * H, 2 * W, 2 * nv), dtype=np.complex128)
    pad[:H, :W, :nv] = psi @ R.T
    return pad


def columns64(H, W, sx, sz, dv):
    """(k [2H, 2W] int64, f [2H, 2W]) of the kernel's columns."""
    sx, sz = FO.f32(sx), FO.f32(sz)
    lb = sx * FO.signed(2 * W).astype(np.float64)
    lc = sz * FO.signed(2 * H).astype(np.float64)
    s = (lb[None, :] * lb[None, :] + lc[:, None] * lc[:, None]) / dv
    kf = np.floor(s)
    return np.minimum(kf, 2.0 ** 40).astype(np.int64), s - kf


def kernel64(H, W, nv, sx, sz, dv, scale=None):
    """(K [2H, 2W, 2nv] float64, scale); scale None: 1 / ||K||_2 of the unscaled kernel."""
    k, f = columns64(H, W, sx, sz, dv)
    K = np.zeros((2 * H, 2 * W, 2 * nv))
    ci, bi = np.nonzero(k <= nv - 1)
    K[ci, bi, k[ci, bi]] = 1.0 - f[ci, bi]
    ci, bi = np.nonzero(k + 1 <= nv - 1)
    K[ci, bi, k[ci, bi] + 1] = f[ci, bi]
    if scale is None:
        scale = 1.0 / np.sqrt((K * K).sum())
    return K * scale, scale


def inverse64(Fk, snr, backprop=False):
    """G from the kernel's spectrum (any complex dtype, taken to complex128 as it is)."""
    Fk = np.asarray(Fk).astype(np.complex128)
    if backprop:
        return np.conj(Fk)
    return np.conj(Fk) / (Fk.real ** 2 + Fk.imag ** 2 + 1.0 / FO.f32(snr))


def store64(o, H, W, R):
    """[W, nr, H] float64: max(R^T Re o, 0) of the [0:H, 0:W, 0:nv] corner, transposed into the voxel order."""
    nv, nr = R.shape
    o = np.asarray(o)[:H, :W, :nv].real.astype(np.float64)
    return np.ascontiguousarray(np.maximum(o @ R, 0.0).transpose(1, 2, 0))


def store_scale64(o, H, W, R):
    """[W, nr, H] float64: sum_i R[i, j] |Re o[m, n, i]|, what the store pass's rounding is relative to."""
    nv, nr = R.shape
    o = np.abs(np.asarray(o)[:H, :W, :nv].real.astype(np.float64))
    return np.ascontiguousarray((o @ R).transpose(1, 2, 0))


def reconstruct64(rows, H, W, sx, sz, r0, dr, power=4, snr=0.8, nv=None, backprop=False, perm=None, x_along="n"):
    """The whole transform, [W, nr, H] float64."""
    nr = np.asarray(rows).shape[1]
    R, dv = resampling64(r0, dr, nr, nv)
    K, _ = kernel64(H, W, R.shape[0], sx, sz, dv)
    G = inverse64(np.fft.fftn(K), snr, backprop)
    S = np.fft.fftn(load64(rows, H, W, r0, dr, R, power, perm, x_along))
    return store64(np.fft.ifftn(S * G), H, W, R)
