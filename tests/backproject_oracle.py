"""Float64 numpy restatement of the back-projection (include/nlosgr.h, ABI 13), fed the same fp32 inputs the
kernel reads, including the fp32 r0 and inv_dr.  For voxel centre x (grid tables) and wall point i:

    d = sqrt(dx*dx + dy*dy + dz*dz),  u = (d - r0) * inv_dr,  k = floor(u),  f = u - k
    s_i = (1-f) h_i[k] + f h_i[k+1],  h_i[j] = 0 for j < 0 or j >= nr
    out(x) = sum_i d^power s_i

and the per-voxel bound the GPU tests hold the fp32 kernel to, with no further factor:

    B(x) = sum_i d^p [ du_i S_i + 264 2^-24 (|h_i[k]| + |h_i[k+1]|) ]

    du_i = 6 2^-24 (d + |r0|) inv_dr   the fp32 error of u: three subtractions, the sum of squares, the sqrt
                                       and the scale
    S_i                                the largest absolute slope of the three intervals around k, so a different
                                       floor on the GPU is covered by the continuity of s_i in u
    264                                8 roundings of the term + 256 of the fp32 tile sum
    the term is taken over -2 <= k <= nr (outside, every interval around k is dark)

The bound is derived, not tuned: a numpy fp32 emulation of the kernel's arithmetic stays at <= 0.016 B (powers
0, 2, 4: test_backproject_cpu.py), while a wrong bin or a wrong weight is orders of magnitude outside it.
"""
import numpy as np

U = 2.0 ** -24
PAD = 4   # zero bins on either side of a row: k - 1 .. k + 2 for -3 <= k <= nr + 1 are all addressable


def coords64(xs, ys, zs):
    """[V, 3] float64 voxel centres in (ix*ny + iy)*nz + iz order from the three fp32 tables."""
    g = np.meshgrid(*(np.asarray(t, dtype=np.float32).astype(np.float64) for t in (xs, ys, zs)), indexing="ij")
    return np.stack(g, axis=-1).reshape(-1, 3)


def distances64(walls, xs, ys, zs):
    """[V, nwall] float64 distances of every voxel centre to every wall point (exact differences of the fp32
    inputs, summed and rooted in float64)."""
    X = coords64(xs, ys, zs)
    W = np.asarray(walls, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    d2 = np.zeros((X.shape[0], W.shape[0]))
    for a in range(3):
        d2 += (X[:, a, None] - W[None, :, a]) ** 2
    return np.sqrt(d2)


def bin_coordinate(d, r0, inv_dr):
    """u = (d - r0) * inv_dr in float64 from the fp32 r0 and inv_dr."""
    return (d - float(np.float32(r0))) * float(np.float32(inv_dr))


def backproject64(rows, walls, xs, ys, zs, r0, inv_dr, power, d=None, want_bound=True):
    """(out [nx,ny,nz] float64, B [nx,ny,nz] float64 or None).  rows [nwall, nr]: the fp32 rows the kernel reads,
    or float64 rows (a float64-filtered capture) taken as they are; NaN / inf propagate into out and B.
    d: distances64 of the same walls and tables when the caller has it."""
    rows = np.asarray(rows)
    nw, nr = rows.shape
    shape = (len(xs), len(ys), len(zs))
    if d is None:
        d = distances64(walls, xs, ys, zs)
    if nw == 0:
        z = np.zeros(shape)
        return z, (z.copy() if want_bound else None)
    u = bin_coordinate(d, r0, inv_dr)
    k = np.floor(u)
    f = u - k
    kc = np.clip(k, -3, nr + 1).astype(np.int64)       # outside [-2, nr] every bin around k is a padding zero
    hp = np.zeros((nw, nr + 2 * PAD))
    hp[:, PAD:PAD + nr] = rows.astype(np.float64)
    idx = kc + PAD
    col = np.arange(nw)[None, :]
    h0, h1 = hp[col, idx], hp[col, idx + 1]
    w = d ** int(power)
    with np.errstate(invalid="ignore"):
        out = (w * ((1.0 - f) * h0 + f * h1)).sum(axis=1)
        if not want_bound:
            return out.reshape(shape), None
        hm, h2 = hp[col, idx - 1], hp[col, idx + 2]
        S = np.maximum(np.maximum(np.abs(h0 - hm), np.abs(h1 - h0)), np.abs(h2 - h1))
        du = 6.0 * U * (d + abs(float(np.float32(r0)))) * float(np.float32(inv_dr))
        term = du * S + 264.0 * U * (np.abs(h0) + np.abs(h1))
        term = np.where((k >= -2) & (k <= nr), term, 0.0)
        B = (w * term).sum(axis=1)
    return out.reshape(shape), B.reshape(shape)


def emulate32(rows, walls, xs, ys, zs, r0, inv_dr, power, tile=256):
    """The kernel's arithmetic in numpy fp32 (every operation rounded to fp32, the distance in the kernel's
    order, the correctly rounded sqrt in place of the hardware's 1-ulp one, no fma), the tile sums in fp32 term
    by term and the tiles in float64: what the bound has to cover besides a different floor."""
    f32 = np.float32
    rows = np.asarray(rows, dtype=f32)
    nw, nr = rows.shape
    g = np.meshgrid(*(np.asarray(t, dtype=f32) for t in (xs, ys, zs)), indexing="ij")
    X = np.stack(g, axis=-1).reshape(-1, 3)
    W = np.asarray(walls, dtype=f32).reshape(-1, 3)
    r0, inv_dr = f32(r0), f32(inv_dr)
    acc = np.zeros(X.shape[0], dtype=np.float64)
    hp = np.zeros((nw, nr + 2 * PAD), dtype=f32)
    hp[:, PAD:PAD + nr] = rows
    for base in range(0, nw, tile):
        s = np.zeros(X.shape[0], dtype=f32)
        for i in range(base, min(nw, base + tile)):
            dx, dy, dz = X[:, 0] - W[i, 0], X[:, 1] - W[i, 1], X[:, 2] - W[i, 2]
            d = np.sqrt((dx * dx + dy * dy) + dz * dz)
            u = np.minimum(np.maximum((d - r0) * inv_dr, f32(-2.0)), f32(nr + 1))
            kf = np.floor(u)
            f = u - kf
            k = kf.astype(np.int64) + PAD
            h0, h1 = hp[i, k], hp[i, k + 1]
            sv = (f32(1.0) - f) * h0 + f * h1
            d2 = d * d
            w = [np.ones_like(d), d, d2, d2 * d, d2 * d2][int(power)]
            s = s + w * sv
        acc += s.astype(np.float64)
    return acc.astype(f32).reshape(len(xs), len(ys), len(zs))


def relay_wall(h, w, extent=1.0):
    """Cell-centred h x w wall points on the plane y = 0 over x, z in [-extent/2, extent/2], row-major
    (nlosgr.geometry.relay_wall_grid's layout) as fp32 [h*w, 3]."""
    zs = (np.arange(h) + 0.5) / h * extent - extent / 2
    xs = (np.arange(w) + 0.5) / w * extent - extent / 2
    zz, xx = np.meshgrid(zs, xs, indexing="ij")
    return np.stack([xx.reshape(-1), np.zeros(h * w), zz.reshape(-1)], axis=1).astype(np.float32)


def linspace_tables(position, size, res):
    """The three fp32 tables of VoxelGrid(position, size, res)."""
    res = (res,) * 3 if np.isscalar(res) else tuple(res)
    return tuple(np.linspace(p - size / 2, p + size / 2, n).astype(np.float32) for p, n in zip(position, res))


# the small scene of the derivation and of the point-scatterer checks: wall 16 x 16, grid 17^3, 80 bins
SCENE = dict(wall=(16, 16), position=(0.0, 0.5, 0.0), size=0.5, res=17, r0=0.2, dr=0.01, nr=80, voxel=(11, 5, 3))


def scene_window():
    """(r0, inv_dr) of SCENE as the fp32 values the kernel gets."""
    return float(np.float32(SCENE["r0"])), float(np.float32(1.0) / np.float32(SCENE["dr"]))


def scatterer_rows(walls, point, r0, inv_dr, nr):
    """[nwall, nr] fp32: every wall point's histogram of one point scatterer, the linear splat (1-f, f) at
    its time of flight (bins outside the window dropped)."""
    W = np.asarray(walls, dtype=np.float32).astype(np.float64)
    p = np.asarray(point, dtype=np.float32).astype(np.float64)
    u = bin_coordinate(np.sqrt(((W - p[None]) ** 2).sum(axis=1)), r0, inv_dr)
    k = np.floor(u).astype(np.int64)
    f = u - k
    rows = np.zeros((W.shape[0], nr))
    for b, v in ((k, 1.0 - f), (k + 1, f)):
        ok = (b >= 0) & (b < nr)
        rows[np.nonzero(ok)[0], b[ok]] += v[ok]
    return rows.astype(np.float32)


def scatterer_scene():
    """(rows, walls, (xs, ys, zs), r0, inv_dr) of the SCENE's point scatterer at voxel SCENE['voxel']."""
    walls = relay_wall(*SCENE["wall"])
    tabs = linspace_tables(SCENE["position"], SCENE["size"], SCENE["res"])
    r0, inv_dr = scene_window()
    i, j, k = SCENE["voxel"]
    p = (tabs[0][i], tabs[1][j], tabs[2][k])
    return scatterer_rows(walls, p, r0, inv_dr, SCENE["nr"]), walls, tabs, r0, inv_dr
