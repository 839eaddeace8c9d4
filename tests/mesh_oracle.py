"""CPU oracle of the isosurface extraction (nlosgr.mesh -> nlosgr_mesh_count / nlosgr_mesh_emit): marching
tetrahedra on the Kuhn decomposition of a regular grid, restated in vectorised numpy.

Classification uses the fp32 values exactly as the kernels do (inside iff isfinite(f) and f >= level), so the
index topology (vertex numbering, faces) is exact; positions, values and normals are float64 arithmetic on
the given fp32 inputs.

Orderings (include/nlosgr.h, "Surface output"):
    corner / direction code   bit 0 = x, bit 1 = y, bit 2 = z
    owned edges of point p    p -> p + d, d0..d6 = (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
    vertices                  one per crossing edge, by owner linear index (ix*ny + iy)*nz + iz, then d
    tetrahedra of a cell      tau = 0..5, axis permutations (a,b,c) in lexicographic order;
                              v0 = p, v1 = v0 + e_a, v2 = v1 + e_b, v3 = p + (1,1,1)
    triangles                 by cell linear index (ix*(ny-1) + iy)*(nz-1) + iz, then tau, then the rule below
"""
import numpy as np

PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
EDGE_DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]


def tet_corners(tau):
    """The four corners of tetrahedron tau as integer offsets from the cell's base point."""
    a, b, _ = PERMS[tau]
    v1 = np.zeros(3, dtype=np.int64)
    v1[a] = 1
    v2 = v1.copy()
    v2[b] = 1
    return [np.zeros(3, dtype=np.int64), v1, v2, np.ones(3, dtype=np.int64)]


def _unwound(mask):
    """Triangles of a corner mask as edges (X, Y) between corner numbers, before the winding rule."""
    ins = [i for i in range(4) if mask >> i & 1]
    outs = [i for i in range(4) if not mask >> i & 1]
    if len(ins) == 1:
        return [[(ins[0], o) for o in outs]]
    if len(ins) == 3:
        return [[(i, outs[0]) for i in ins]]
    if len(ins) == 2:
        (A, B), (C, D) = ins, outs
        return [[(A, C), (A, D), (B, D)], [(A, C), (B, D), (B, C)]]
    return []


def tet_table():
    """TABLE[tau][mask]: list of triangles, each three edges (X, Y), X < Y in corner order (X's point is the
    componentwise smaller one: the owner), wound by the midpoint rule: with the crossings at the edge
    midpoints of the unit cell, the last two vertices are swapped iff
    (p1 - p0) x (p2 - p0) . (mean of outside corners - mean of inside corners) < 0."""
    table = []
    for tau in range(6):
        v = [c.astype(np.float64) for c in tet_corners(tau)]
        row = []
        for mask in range(16):
            ins = [i for i in range(4) if mask >> i & 1]
            outs = [i for i in range(4) if not mask >> i & 1]
            tris = []
            for tri in _unwound(mask):
                p = [(v[x] + v[y]) / 2 for x, y in tri]
                direction = np.mean([v[i] for i in outs], axis=0) - np.mean([v[i] for i in ins], axis=0)
                s = np.dot(np.cross(p[1] - p[0], p[2] - p[0]), direction)
                assert s != 0.0, (tau, mask)
                if s < 0:
                    tri = [tri[0], tri[2], tri[1]]
                tris.append([tuple(sorted(e)) for e in tri])
            row.append(tris)
        table.append(row)
    return table


TABLE = tet_table()
_DIDX = {d: i for i, d in enumerate(EDGE_DIRS)}


def inside_mask(f, level):
    f = np.asarray(f)
    assert f.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return np.isfinite(f) & (f >= np.float32(level))


def corner_configurations(f, level):
    """Histogram [256] of the 8-corner inside patterns over all cells (bit = x + 2y + 4z of the corner)."""
    ins = inside_mask(f, level)
    nx, ny, nz = ins.shape
    code = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        ox, oy, oz = c & 1, c >> 1 & 1, c >> 2 & 1
        code |= ins[ox:nx - 1 + ox, oy:ny - 1 + oy, oz:nz - 1 + oz].astype(np.int64) << c
    return np.bincount(code.ravel(), minlength=256)


def _gradient(f64, tables):
    """[nx,ny,nz,3]: (f[i+1] - f[i-1]) / (x[i+1] - x[i-1]) per axis, one-sided at the two ends."""
    g = np.zeros(f64.shape + (3,))
    for ax in range(3):
        n = f64.shape[ax]
        x = np.asarray(tables[ax], dtype=np.float64)
        lo = np.maximum(np.arange(n) - 1, 0)
        hi = np.minimum(np.arange(n) + 1, n - 1)
        shape = [1, 1, 1]
        shape[ax] = n
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            g[..., ax] = (np.take(f64, hi, axis=ax) - np.take(f64, lo, axis=ax)) / (x[hi] - x[lo]).reshape(shape)
    return g


def extract(f, tables, level, values=None):
    """Mesh of {f = level}.  f [nx,ny,nz] fp32, tables three fp32 coordinate arrays, values optional fp32
    volume.  Returns a dict: vertices [nv,3] f64, normals [nv,3] f64, values [nv] f64 | None, faces [nt,3]
    int32, and per vertex: t, owner (linear index), d (edge number), gnorm (length of the interpolated
    gradient), gmax (largest grid gradient length, a scalar)."""
    f = np.ascontiguousarray(f)
    assert f.dtype == np.float32 and f.ndim == 3
    tables = [np.asarray(t) for t in tables]
    assert all(t.dtype == np.float32 for t in tables)
    nx, ny, nz = f.shape
    empty = {"vertices": np.zeros((0, 3)), "normals": np.zeros((0, 3)),
             "values": None if values is None else np.zeros(0), "faces": np.zeros((0, 3), dtype=np.int32),
             "t": np.zeros(0), "owner": np.zeros(0, dtype=np.int64), "d": np.zeros(0, dtype=np.int64),
             "gnorm": np.zeros(0), "gmax": 0.0}
    if min(nx, ny, nz) < 2:
        return empty
    ins = inside_mask(f, level)
    lvl = np.float64(np.float32(level))
    f64 = f.astype(np.float64)
    cross = np.zeros((nx, ny, nz, 7), dtype=bool)
    for k, (dx, dy, dz) in enumerate(EDGE_DIRS):
        cross[:nx - dx, :ny - dy, :nz - dz, k] = ins[:nx - dx, :ny - dy, :nz - dz] != ins[dx:, dy:, dz:]
    flat = cross.reshape(-1)
    vid = (np.cumsum(flat) - 1).reshape(cross.shape)
    nv = int(flat.sum())
    sel = np.nonzero(flat)[0]
    owner, d = sel // 7, sel % 7
    oi = np.stack(np.unravel_index(owner, (nx, ny, nz)), axis=1)
    fi = oi + np.asarray(EDGE_DIRS)[d]
    fa, fb = f64[tuple(oi.T)], f64[tuple(fi.T)]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (lvl - fa) / (fb - fa)
    t = np.where(np.isfinite(fa) & np.isfinite(fb), t, 0.5)
    X = [t_.astype(np.float64) for t_ in tables]
    xa = np.stack([X[ax][oi[:, ax]] for ax in range(3)], axis=1)
    xb = np.stack([X[ax][fi[:, ax]] for ax in range(3)], axis=1)
    verts = xa + t[:, None] * (xb - xa)
    vals = None
    if values is not None:
        a64 = np.asarray(values, dtype=np.float32).astype(np.float64)
        aa, ab = a64[tuple(oi.T)], a64[tuple(fi.T)]
        vals = aa + t * (ab - aa)
    g = _gradient(f64, tables)
    ga, gb = g[tuple(oi.T)], g[tuple(fi.T)]
    with np.errstate(invalid="ignore", over="ignore"):
        gv = ga + t[:, None] * (gb - ga)
        gn = np.sqrt((gv * gv).sum(axis=1))
        ok = np.isfinite(gn) & (gn > 0)
        normals = np.where(ok[:, None], -gv / np.where(ok, gn, 1.0)[:, None], 0.0)
        gl = np.sqrt((g * g).sum(axis=-1))
    gmax = float(gl[np.isfinite(gl)].max()) if np.isfinite(gl).any() else 0.0

    cx, cy, cz = nx - 1, ny - 1, nz - 1
    keys, tris = [], []
    cell_lin = np.arange(cx * cy * cz).reshape(cx, cy, cz)
    for tau in range(6):
        cor = tet_corners(tau)
        mask = np.zeros((cx, cy, cz), dtype=np.int64)
        for i, c in enumerate(cor):
            mask |= ins[c[0]:cx + c[0], c[1]:cy + c[1], c[2]:cz + c[2]].astype(np.int64) << i
        for m in range(1, 15):
            cells = np.nonzero(mask == m)
            if cells[0].size == 0:
                continue
            for k, tri in enumerate(TABLE[tau][m]):
                ids = []
                for x, y in tri:
                    o = cor[x]
                    dd = _DIDX[tuple(int(v) for v in cor[y] - cor[x])]
                    ids.append(vid[cells[0] + o[0], cells[1] + o[1], cells[2] + o[2], dd])
                tris.append(np.stack(ids, axis=1))
                keys.append((cell_lin[cells] * 6 + tau) * 2 + k)
    if tris:
        keys, tris = np.concatenate(keys), np.concatenate(tris)
        faces = tris[np.argsort(keys, kind="stable")].astype(np.int32)
    else:
        faces = np.zeros((0, 3), dtype=np.int32)
    assert faces.size == 0 or (faces.min() >= 0 and faces.max() < nv)
    return {"vertices": verts, "normals": normals, "values": vals, "faces": faces, "t": t, "owner": owner, "d": d,
            "gnorm": np.where(np.isfinite(gn), gn, 0.0), "gmax": gmax}


# ---------------------------------------------------------------------------------------------------
# topology helpers (index topology only: zero-area triangles count like any other)
# ---------------------------------------------------------------------------------------------------
def _directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)


def edge_counts(faces):
    """(unique undirected edges [ne,2], how many faces use each)."""
    e = np.sort(_directed_edges(faces), axis=1)
    if e.shape[0] == 0:
        return e, np.zeros(0, dtype=np.int64)
    return np.unique(e, axis=0, return_counts=True)


def boundary_edges(faces):
    """Undirected edges used by exactly one face."""
    e, c = edge_counts(faces)
    return e[c == 1]


def is_edge_manifold(faces, closed=True):
    """Every undirected edge is used by two faces (one or two when not closed), never more, and the two
    uses run in opposite directions (consistent orientation)."""
    e, c = edge_counts(faces)
    if (c > 2).any() or (closed and (c != 2).any()):
        return False
    de = _directed_edges(faces)
    _, dc = np.unique(de, axis=0, return_counts=True)
    return bool((dc == 1).all())


def euler_characteristic(faces):
    """V - E + F over the vertices the faces reference."""
    e, _ = edge_counts(faces)
    return int(np.unique(np.asarray(faces)).size - e.shape[0] + np.asarray(faces).shape[0])


def signed_volume(vertices, faces):
    """Sum of det(p0, p1, p2) / 6: positive for a closed mesh wound counter-clockwise seen from outside."""
    v = np.asarray(vertices, dtype=np.float64)
    p0, p1, p2 = (v[np.asarray(faces)[:, i]] for i in range(3))
    return float(np.einsum("ij,ij->i", p0, np.cross(p1, p2)).sum() / 6.0)


def triangle_areas(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    p0, p1, p2 = (v[np.asarray(faces)[:, i]] for i in range(3))
    return 0.5 * np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1)


def unreferenced_vertices(nv, faces):
    used = np.zeros(nv, dtype=bool)
    used[np.asarray(faces).ravel()] = True
    return int((~used).sum())


# ---------------------------------------------------------------------------------------------------
# shared test volumes
# ---------------------------------------------------------------------------------------------------
def linspace_tables(axes):
    """fp32 tables from (lo, hi, n) triples, built as nlosgr.voxelize.VoxelGrid builds them."""
    return [np.linspace(float(lo), float(hi), int(n)).astype(np.float32) for lo, hi, n in axes]


def gaussian_field(tables, centre, inv_cov_half, amp=1.0):
    """amp * exp(-d^T M d) on the grid, d = x - centre, M = inv_cov_half [3,3] (float64, returned fp32)."""
    X = np.stack(np.meshgrid(*(t.astype(np.float64) for t in tables), indexing="ij"), axis=-1) - np.asarray(centre)
    q = np.einsum("...i,ij,...j->...", X, np.asarray(inv_cov_half, dtype=np.float64), X)
    return (amp * np.exp(-q)).astype(np.float32)


NOISE_SHAPE = (9, 17, 70)
NOISE_AXES = ((-0.3, 0.4, 9), (0.2, 1.1, 17), (-1.0, 2.5, 70))   # three different spacings


def noise_case():
    """standard_normal seed 0, 9x17x70, on non-uniform-extent tables; level 0."""
    f = np.random.default_rng(0).standard_normal(NOISE_SHAPE).astype(np.float32)
    a = np.random.default_rng(1).standard_normal(NOISE_SHAPE).astype(np.float32)
    return f, a, linspace_tables(NOISE_AXES)


BLOB_SHAPE = (24, 20, 28)
BLOB_AXES = ((-0.25, 0.25, 24), (0.25, 0.75, 20), (-0.25, 0.25, 28))   # the hidden-volume box


def blobs_case():
    """Three anisotropic analytic Gaussians summed on 24x20x28 over the hidden-volume box, and a smooth
    second field to interpolate values from."""
    tabs = linspace_tables(BLOB_AXES)
    rot = lambda a: np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    M = lambda s, a: rot(a) @ np.diag(0.5 / np.asarray(s, dtype=np.float64) ** 2) @ rot(a).T
    f = (gaussian_field(tabs, (-0.05, 0.47, -0.04), M((0.05, 0.035, 0.055), 0.4), 1.0).astype(np.float64) +
         gaussian_field(tabs, (0.06, 0.54, 0.05), M((0.035, 0.05, 0.04), -0.7), 0.8) +
         gaussian_field(tabs, (0.01, 0.44, 0.08), M((0.04, 0.03, 0.035), 1.1), 0.6)).astype(np.float32)
    X = np.stack(np.meshgrid(*(t.astype(np.float64) for t in tabs), indexing="ij"), axis=-1)
    a = (0.5 + X[..., 0] - 2.0 * X[..., 1] * X[..., 2]).astype(np.float32)
    return f, a, tabs


def exact_case():
    """Integer-valued 7x6x5 volume (integers(0, 4), seed 0); level 2 hits corners exactly."""
    f = np.random.default_rng(0).integers(0, 4, size=(7, 6, 5)).astype(np.float32)
    return f, linspace_tables(((0.0, 1.2, 7), (-0.5, 0.5, 6), (1.0, 3.0, 5)))
