"""Float64 numpy restatement of f-k migration (include/nlosgr.h, the nlosgr_fk_* symbols), fed the same fp32 inputs
the kernels read: the fp32 rows and the fp32 r0, dr, sx, sz.  Each of the three stages is callable alone.

Input: rows [H W, nr], the row of lattice point v = m W + n (x_along "n"; "m": v = n H + m) being rows[perm[v]]; the
point is measured at (xs[n], y0, zs[m]).  Nz = 2 H, Nx = 2 W, Nt = 2 nr.

    load    psi[m, n, j] = max(rows[v, j], 0) (r0 + j dr)^power, its square root with `amplitude`, at [0:H, 0:W, 0:nr]
            of a zero array [Nz, Nx, Nt]
            S = fftn(pad)                                               (numpy: unnormalised, exp(-2 pi i ...))
    stolt   signed DFT indices c (z), b (x), a (time); gx = Nt dr / (Nx sx), gz = Nt dr / (Nz sz)
            src = sqrt(a^2 + (gx b)^2 + (gz c)^2), k = floor(src), f = src - k
            V[c, b, a] = ((1-f) S[c, b, k] + f S[c, b, k+1]) a / src exp(-2 pi i (src - a) (r0 / dr) / Nt)
            where a > 0 and k + 1 <= Nt/2 - 1, V = 0 everywhere else
            o = ifftn(V)                                                (1/N)
    store   volume[n, j, m] = |o[m, n, j]|^2 for m < H, n < W, j < nr:  [W, nr, H]

Voxel (n, j, m) is the point (xs[n], y0 + r0 + j dr, zs[m]).
"""
import numpy as np

import backproject_oracle as BO


def f32(v):
    """A scalar as the fp32 value the kernels get, in float64."""
    return float(np.float32(v))


def lattice_rows(H, W, perm=None, x_along="n"):
    """[H, W] int: the row of `rows` that holds lattice point (m, n)."""
    m, n = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    v = m * W + n if x_along == "n" else n * H + m
    return v if perm is None else np.asarray(perm, dtype=np.int64)[v]


def load64(rows, H, W, r0, dr, power=4, amplitude=True, perm=None, x_along="n"):
    """The padded array [2H, 2W, 2nr], complex128 (imaginary part zero)."""
    rows = np.asarray(rows, dtype=np.float32).astype(np.float64)
    nr = rows.shape[1]
    r = f32(r0) + np.arange(nr) * f32(dr)
    psi = np.maximum(rows[lattice_rows(H, W, perm, x_along)], 0.0) * r[None, None, :] ** int(power)
    if amplitude:
        psi = np.sqrt(psi)
    pad = np.zeros((2 * H, 2 * W, 2 * nr), dtype=np.complex128)
    pad[:H, :W, :nr] = psi
    return pad


def signed(N):
    """The signed DFT indices of an axis of even length N: 0 .. N/2 - 1, -N/2 .. -1."""
    i = np.arange(N)
    return np.where(i < N // 2, i, i - N)


def stolt64(S, sx, sz, r0, dr):
    """V [Nz, Nx, Nt] complex128 from the spectrum S (any complex dtype, taken to complex128 as it is)."""
    S = np.asarray(S).astype(np.complex128)
    Nz, Nx, Nt = S.shape
    sx, sz, r0, dr = f32(sx), f32(sz), f32(r0), f32(dr)
    gx, gz = Nt * dr / (Nx * sx), Nt * dr / (Nz * sz)
    c, b, a = np.meshgrid(signed(Nz), signed(Nx), signed(Nt), indexing="ij")
    src = np.sqrt(a.astype(np.float64) ** 2 + (gx * b) ** 2 + (gz * c) ** 2)
    k = np.floor(src).astype(np.int64)
    f = src - k
    ok = (a > 0) & (k + 1 <= Nt // 2 - 1)
    kc = np.where(ok, k, 0)
    S0, S1 = np.take_along_axis(S, kc, axis=2), np.take_along_axis(S, kc + 1, axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        V = ((1.0 - f) * S0 + f * S1) * (a / src) * np.exp(-2j * np.pi * (src - a) * (r0 / dr) / Nt)
    return np.where(ok, V, 0.0)


def store64(o, H, W, nr):
    """[W, nr, H] float64: |o|^2 of the [0:H, 0:W, 0:nr] corner, transposed into the voxel order."""
    o = np.asarray(o)[:H, :W, :nr].astype(np.complex128)
    return np.ascontiguousarray((o.real ** 2 + o.imag ** 2).transpose(1, 2, 0))


def migrate64(rows, H, W, sx, sz, r0, dr, power=4, amplitude=True, perm=None, x_along="n"):
    """The whole transform, [W, nr, H] float64."""
    nr = np.asarray(rows).shape[1]
    S = np.fft.fftn(load64(rows, H, W, r0, dr, power, amplitude, perm, x_along))
    return store64(np.fft.ifftn(stolt64(S, sx, sz, r0, dr)), H, W, nr)


# ---- lattices and their inputs -------------------------------------------------------------------------------

def lattice(H, W, sx, sz):
    """(xs [W], zs [H]) fp32, centred on 0; and the wall points [H W, 3] fp32 on y = 0, row-major (m W + n)."""
    xs = ((np.arange(W) - (W - 1) / 2) * sx).astype(np.float32)
    zs = ((np.arange(H) - (H - 1) / 2) * sz).astype(np.float32)
    zz, xx = np.meshgrid(zs, xs, indexing="ij")
    walls = np.stack([xx.reshape(-1), np.zeros(H * W, dtype=np.float32), zz.reshape(-1)], axis=1).astype(np.float32)
    return xs, zs, walls


# the four point-scatterer lattices: (H, W, nr), spacings, bin width, r0 in bins, the scatterer's voxel (n, j, m)
SCATTERERS = {
    "16x16x64": dict(H=16, W=16, nr=64, sx=0.0625, sz=0.0625, dr=0.02, r0_bins=0, voxel=(10, 30, 5)),
    "12x20x48": dict(H=12, W=20, nr=48, sx=0.05, sz=0.08, dr=0.02, r0_bins=0, voxel=(7, 25, 8)),
    "16x16x64_r20": dict(H=16, W=16, nr=64, sx=0.0625, sz=0.0625, dr=0.02, r0_bins=20, voxel=(10, 12, 5)),
    "16x16x64_r35": dict(H=16, W=16, nr=64, sx=0.0625, sz=0.0625, dr=0.02, r0_bins=35, voxel=(6, 8, 9)),
}


def scatterer_scene(c):
    """(rows [H W, nr] fp32, xs, zs, r0, dr) of one point scatterer at the lattice's voxel c["voxel"]: every wall
    point's histogram is the back-projection's own (k, f) splat at its distance d, weighted d^-4."""
    xs, zs, walls = lattice(c["H"], c["W"], c["sx"], c["sz"])
    dr = f32(c["dr"])
    r0 = f32(c["r0_bins"] * c["dr"])
    n, j, m = c["voxel"]
    point = np.array([xs[n], np.float32(r0 + j * dr), zs[m]], dtype=np.float32)
    inv_dr = float(np.float32(1.0) / np.float32(dr))
    rows = BO.scatterer_rows(walls, point, r0, inv_dr, c["nr"]).astype(np.float64)
    d = np.sqrt(((walls.astype(np.float64) - point.astype(np.float64)[None]) ** 2).sum(axis=1))
    return (rows / d[:, None] ** 4).astype(np.float32), xs, zs, r0, dr


def peak(vol):
    """(argmax as an index triple, peak / median) of a volume."""
    at = tuple(int(v) for v in np.unravel_index(int(np.argmax(vol)), vol.shape))
    return at, float(vol.max() / np.median(vol))


# the dense cases of the GPU tests: (H, W, nr), spacings, bin width, r0 in bins
DENSE = {
    "16x16x64": dict(H=16, W=16, nr=64, sx=0.0625, sz=0.0625, dr=0.02, r0_bins=0),
    "12x20x48": dict(H=12, W=20, nr=48, sx=0.05, sz=0.08, dr=0.02, r0_bins=0),
    "5x7x17_r3": dict(H=5, W=7, nr=17, sx=0.1, sz=0.12, dr=0.03, r0_bins=3),
    "16x16x64_r35": dict(H=16, W=16, nr=64, sx=0.0625, sz=0.0625, dr=0.02, r0_bins=35),
    "1x9x16": dict(H=1, W=9, nr=16, sx=0.1, sz=0.1, dr=0.04, r0_bins=0),
}


def dense_rows(c, seed=5):
    """Seeded dense rows [H W, nr] fp32, non-negative but for a few negative entries (the clamp is hit), so every
    spectrum bin is exercised."""
    g = np.random.default_rng(seed + c["H"] * 1000 + c["W"] * 10 + c["nr"])
    rows = g.random((c["H"] * c["W"], c["nr"])) + 0.05
    neg = g.random(rows.shape) < 0.02
    rows[neg] = -rows[neg]
    return rows.astype(np.float32)


def window(c):
    """(r0, dr) of a case as the fp32 values the kernels get."""
    return f32(c["r0_bins"] * c["dr"]), f32(c["dr"])
