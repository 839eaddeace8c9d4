"""CPU-only checks of the surface output (nlosgr.mesh): the marching-tetrahedra oracle (tests/mesh_oracle.py)
against the invariants a correct extraction has, the PLY round trip, host-side validation of the three C
entry points, and the Python surface's refusals.  No GPU is touched."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mesh_oracle as MO

SPHERE_C = (0.07, -0.04, 0.11)   # off-centre, on no grid plane
SPHERE_R, SPHERE_S = 0.6, 0.5    # iso radius, Gaussian std


def _sphere(n):
    tabs = MO.linspace_tables(((-1.0, 1.0, n),) * 3)
    f = MO.gaussian_field(tabs, SPHERE_C, np.eye(3) * 0.5 / SPHERE_S ** 2)
    return f, tabs, float(np.exp(-0.5 * SPHERE_R ** 2 / SPHERE_S ** 2))


def _torus(n=24, R=0.55, r=0.22):
    tabs = MO.linspace_tables(((-1.0, 1.0, n),) * 3)
    X = np.stack(np.meshgrid(*(t.astype(np.float64) for t in tabs), indexing="ij"), axis=-1) - np.asarray(SPHERE_C)
    d2 = (np.hypot(X[..., 0], X[..., 1]) - R) ** 2 + X[..., 2] ** 2
    return np.exp(-0.5 * d2 / r ** 2).astype(np.float32), tabs, float(np.exp(-0.5))


def test_winding_table_is_generated_and_consistent():
    """6x16 table by the midpoint rule: masks 0 and 15 emit nothing, one / three inside one triangle, two inside
    two; the two triangles of a quad share their diagonal in opposite directions; complementary masks give the
    same triangles with the opposite winding."""
    assert len(MO.TABLE) == 6 and all(len(r) == 16 for r in MO.TABLE)
    for tau in range(6):
        assert MO.TABLE[tau][0] == [] and MO.TABLE[tau][15] == []
        for m in range(1, 15):
            tris = MO.TABLE[tau][m]
            assert len(tris) == (2 if bin(m).count("1") == 2 else 1)
            if len(tris) == 2:
                d0 = {(tris[0][i], tris[0][(i + 1) % 3]) for i in range(3)}
                d1 = {(tris[1][(i + 1) % 3], tris[1][i]) for i in range(3)}
                assert len(d0 & d1) == 1
            for k, tri in enumerate(tris):
                other = MO.TABLE[tau][15 - m]
                rev = [tri[0], tri[2], tri[1]]
                rots = lambda t: [t[i:] + t[:i] for i in range(3)]
                assert any(rev in rots(o) for o in other), (tau, m, k)


def test_sphere_invariants():
    """Off-centre isotropic Gaussian, iso radius 0.6 on [-1,1]^3: closed, Euler characteristic 2, positive
    signed volume, no unreferenced vertex; at 20^3 the enclosed volume and the vertex radii lie in bands taken
    from the oracle's own run (12^3: 0.96345, 20^3: 0.98798, 32^3: 0.99550 of 4/3 pi r^3 -- the chords of a
    convex surface lie inside it; radii at 20^3 within [0.98872, 1.00522] r), with a small margin."""
    for n in (12, 20, 32):
        f, tabs, level = _sphere(n)
        m = MO.extract(f, tabs, level)
        vol = MO.signed_volume(m["vertices"], m["faces"]) / (4.0 / 3.0 * np.pi * SPHERE_R ** 3)
        rad = np.linalg.norm(m["vertices"] - np.asarray(SPHERE_C), axis=1) / SPHERE_R
        print(f"{n}^3: {m['vertices'].shape[0]} vertices, {m['faces'].shape[0]} triangles, volume ratio {vol:.5f}, "
              f"radii [{rad.min():.5f}, {rad.max():.5f}] r")
        assert MO.is_edge_manifold(m["faces"]) and MO.boundary_edges(m["faces"]).shape[0] == 0
        assert MO.euler_characteristic(m["faces"]) == 2
        assert MO.unreferenced_vertices(m["vertices"].shape[0], m["faces"]) == 0
        assert vol > 0
        if n == 20:
            assert 0.985 <= vol <= 0.991
            assert 0.987 <= rad.min() and rad.max() <= 1.007
        # normals point outwards (from high density to low) and are unit
        out = m["vertices"] - np.asarray(SPHERE_C)
        assert (np.einsum("ij,ij->i", m["normals"], out) > 0).all()
        np.testing.assert_allclose(np.linalg.norm(m["normals"], axis=1), 1.0, atol=1e-12)
        # every non-degenerate triangle is counter-clockwise seen from the low-density side
        p0, p1, p2 = (m["vertices"][m["faces"][:, i]] for i in range(3))
        fn = np.cross(p1 - p0, p2 - p0)
        assert (np.einsum("ij,ij->i", fn, (p0 + p1 + p2) / 3 - np.asarray(SPHERE_C)) > 0).all()
    vols = []
    for n in (12, 20, 32):
        f, tabs, level = _sphere(n)
        m = MO.extract(f, tabs, level)
        vols.append(MO.signed_volume(m["vertices"], m["faces"]))
    assert vols[0] < vols[1] < vols[2] < 4.0 / 3.0 * np.pi * SPHERE_R ** 3   # converges from inside


def test_two_blobs_and_torus_topology():
    tabs = MO.linspace_tables(((-1.0, 1.0, 24),) * 3)
    M = np.eye(3) * 0.5 / 0.2 ** 2
    f = (MO.gaussian_field(tabs, (-0.45, 0.03, 0.02), M).astype(np.float64) +
         MO.gaussian_field(tabs, (0.47, -0.05, 0.04), M)).astype(np.float32)
    m = MO.extract(f, tabs, 0.4)
    chi, vol = MO.euler_characteristic(m["faces"]), MO.signed_volume(m["vertices"], m["faces"])
    print(f"two blobs: chi {chi}, signed volume {vol:.5f}")
    assert MO.is_edge_manifold(m["faces"]) and chi == 4 and vol > 0
    f, tabs, level = _torus()
    m = MO.extract(f, tabs, level)
    chi, vol = MO.euler_characteristic(m["faces"]), MO.signed_volume(m["vertices"], m["faces"])
    print(f"torus: chi {chi}, signed volume {vol:.5f}")
    assert MO.is_edge_manifold(m["faces"]) and chi == 0 and vol > 0
    assert MO.unreferenced_vertices(m["vertices"].shape[0], m["faces"]) == 0


def test_surface_cut_by_the_grid_has_boundary_only_on_outer_faces():
    """A Gaussian centred near the x = lo face: the mesh is open, manifold, and both ends of every boundary
    edge lie on an outer face of the grid."""
    tabs = MO.linspace_tables(((-1.0, 1.0, 16), (-1.0, 1.0, 14), (-1.0, 1.0, 15)))
    f = MO.gaussian_field(tabs, (-0.93, 0.05, 0.1), np.eye(3) * 0.5 / 0.4 ** 2)
    m = MO.extract(f, tabs, 0.5)
    b = MO.boundary_edges(m["faces"])
    assert b.shape[0] > 0 and MO.is_edge_manifold(m["faces"], closed=False)
    lo, hi = np.array([t[0] for t in tabs], dtype=np.float64), np.array([t[-1] for t in tabs], dtype=np.float64)
    on_face = ((m["vertices"] == lo) | (m["vertices"] == hi)).any(axis=1)
    assert on_face[b.ravel()].all()
    assert (m["vertices"][b.ravel(), 0] == lo[0]).all()      # here: the x = lo face only
    assert MO.unreferenced_vertices(m["vertices"].shape[0], m["faces"]) == 0


def test_noise_and_exact_hit_counts():
    """The figures of the shared GPU cases, from the oracle alone: 9x17x70 standard_normal at level 0 shows
    all 256 corner configurations, 33 556 vertices and 66 150 triangles; the integer 7x6x5 volume at level 2
    stays finite and index-manifold with 346 zero-area triangles."""
    f, a, tabs = MO.noise_case()
    hist = MO.corner_configurations(f, 0.0)
    m = MO.extract(f, tabs, 0.0, a)
    print(f"noise: rarest configuration {hist.min()} times; {m['vertices'].shape[0]} vertices, {m['faces'].shape[0]} triangles")
    assert (hist > 0).all()
    assert m["vertices"].shape[0] == 33556 and m["faces"].shape[0] == 66150
    assert MO.unreferenced_vertices(33556, m["faces"]) == 0
    assert MO.is_edge_manifold(m["faces"], closed=False)
    f, tabs = MO.exact_case()
    m = MO.extract(f, tabs, 2.0)
    zero = int((MO.triangle_areas(m["vertices"], m["faces"]) == 0).sum())
    print(f"exact hits: {m['faces'].shape[0]} triangles, {zero} of zero area")
    assert np.isfinite(m["vertices"]).all() and zero == 346
    assert MO.is_edge_manifold(m["faces"], closed=False)
    assert MO.extract(f[:1], [tabs[0][:1], tabs[1], tabs[2]], 2.0)["faces"].shape == (0, 3)   # an extent < 2


def test_ply_round_trip_is_bitwise(tmp_path):
    from nlosgr.mesh import Mesh, read_ply, write_ply
    f, a, tabs = MO.blobs_case()
    m = MO.extract(f, tabs, 0.3, a)
    v, n, s = (m[k].astype(np.float32) for k in ("vertices", "normals", "values"))
    v[0, 0], s[1] = np.float32("nan"), np.float32("-inf")       # any bit pattern survives
    for vals in (s, None):
        path = str(tmp_path / "m.ply")
        write_ply(path, Mesh(torch.from_numpy(v), torch.from_numpy(n), None if vals is None else torch.from_numpy(vals),
                             torch.from_numpy(m["faces"])))
        raw = open(path, "rb").read()
        head = raw[:raw.index(b"end_header\n")].decode("ascii").split("\n")
        assert head[:2] == ["ply", "format binary_little_endian 1.0"]
        assert f"element vertex {v.shape[0]}" in head and f"element face {m['faces'].shape[0]}" in head
        props = [h.split()[-1] for h in head if h.startswith("property float")]
        assert props == ["x", "y", "z", "nx", "ny", "nz"] + (["value"] if vals is not None else [])
        assert "property list uchar int vertex_indices" in head
        body = len(raw) - raw.index(b"end_header\n") - len(b"end_header\n")
        assert body == v.shape[0] * 4 * len(props) + m["faces"].shape[0] * 13
        back = read_ply(path)
        assert back.vertices.tobytes() == v.tobytes() and back.normals.tobytes() == n.tobytes()
        assert back.faces.dtype == np.int32 and np.array_equal(back.faces, m["faces"])
        assert (back.values is None) if vals is None else (back.values.tobytes() == vals.tobytes())
    write_ply(path, Mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), None, np.zeros((0, 3), np.int32)))
    back = read_ply(path)
    assert back.vertices.shape == (0, 3) and back.faces.shape == (0, 3) and back.values is None


def test_mesh_entry_points_validate_on_the_host():
    """Argument validation of nlosgr_mesh_workspace_bytes / nlosgr_mesh_count / nlosgr_mesh_emit runs on the host
    before any launch and reports through nlosgr_last_error (no GPU; fake non-null pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    V = lambda nx=8, ny=8, nz=8, p=fake: _lib.VoxelGrid(nx, ny, nz, p, p, p)
    count = lambda vol=fake, v=None, ws=fake, out=fake: lib.nlosgr_mesh_count(vol, v or V(), 0.5, ws, out, None)

    def emit(vol=fake, attr=None, v=None, ws=fake, nv=10, nt=20, verts=fake, normals=fake, aout=None, tris=fake):
        return lib.nlosgr_mesh_emit(vol, attr, v or V(), 0.5, ws, nv, nt, verts, normals, aout, tris, None)

    n = 8 * 8 * 8
    assert lib.nlosgr_mesh_workspace_bytes(V()) >= 12 * n
    assert lib.nlosgr_mesh_workspace_bytes(V(1, 5, 5)) > 0                    # a valid grid with an empty mesh
    assert lib.nlosgr_mesh_workspace_bytes(V(1024, 2, 1024)) >= 12 * 2 * 1024 * 1024
    assert lib.nlosgr_mesh_workspace_bytes(None) == 0 and b"null" in lib.nlosgr_last_error()
    assert lib.nlosgr_mesh_workspace_bytes(V(p=None)) == 0 and b"table" in lib.nlosgr_last_error()
    for bad in (dict(nx=0), dict(ny=0), dict(nz=-2), dict(nx=1025), dict(nz=4096)):
        assert lib.nlosgr_mesh_workspace_bytes(V(**bad)) == 0 and b"1..1024" in lib.nlosgr_last_error(), bad
        assert count(v=V(**bad)) == 1 and b"1..1024" in lib.nlosgr_last_error(), bad
        assert emit(v=V(**bad)) == 1 and b"1..1024" in lib.nlosgr_last_error(), bad
    assert count(v=V(p=None)) == 1 and b"table" in lib.nlosgr_last_error()
    assert count(vol=None) == 1 and b"null volume" in lib.nlosgr_last_error()
    assert count(ws=None) == 1 and b"workspace" in lib.nlosgr_last_error()
    assert count(out=None) == 1 and b"counts" in lib.nlosgr_last_error()
    assert lib.nlosgr_mesh_count(fake, None, 0.5, fake, fake, None) == 1
    assert emit(v=V(p=None)) == 1 and b"table" in lib.nlosgr_last_error()
    assert emit(vol=None) == 1 and b"null volume" in lib.nlosgr_last_error()
    assert emit(ws=None) == 1 and b"workspace" in lib.nlosgr_last_error()
    assert emit(nv=-1) == 1 and emit(nt=-1) == 1
    assert emit(nv=2 ** 31) == 3 and b"2^31" in lib.nlosgr_last_error()
    assert emit(nt=2 ** 31) == 3 and emit(nv=2 ** 40, nt=2 ** 40) == 3
    assert emit(verts=None) == 1 and b"vertex output" in lib.nlosgr_last_error()
    assert emit(tris=None) == 1 and b"triangle output" in lib.nlosgr_last_error()
    assert emit(attr=fake) == 1 and b"attr" in lib.nlosgr_last_error()         # attr without attr_out
    assert emit(aout=fake) == 1 and b"attr" in lib.nlosgr_last_error()         # attr_out without attr
    assert emit(nv=0, nt=0, verts=None, normals=None, tris=None) == 0          # an empty mesh: nothing to write
    assert emit(v=V(1, 5, 5), nv=0, nt=0, verts=None, tris=None) == 0


def test_isosurface_refuses_cpu_tensors():
    import nlosgr
    from nlosgr.mesh import extract_mesh, isosurface
    from nlosgr.voxelize import VoxelGrid
    assert nlosgr.isosurface is isosurface and nlosgr.extract_mesh is extract_mesh
    grid = VoxelGrid((0, 0.5, 0), 0.5, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        isosurface(torch.zeros(4, 4, 4), grid, 0.5)
    with pytest.raises(RuntimeError, match="GPU"):
        extract_mesh(nlosgr.GaussianParams.synthetic(8, 1, preset="cuda", seed=1), grid, torch.zeros(3))
    with pytest.raises(ValueError):
        extract_mesh(None, grid, None, field="colour")
    with pytest.raises(ValueError):
        extract_mesh(None, grid, None, level=1.0, level_frac=0.5)


def test_gaussian2volume_modes():
    """'mesh' (the Poisson route) still raises NotImplementedError naming open3d and now points at 'isosurface';
    unknown modes still raise ValueError; 'isosurface' is a known mode (without a GPU it fails in voxelize)."""
    from nlosgr import nlos_helpers as NH
    with pytest.raises(NotImplementedError, match="open3d") as e:
        NH.gaussian2volume(SimpleNamespace(), None, {}, None, resolution=8, mode="mesh")
    assert "isosurface" in str(e.value)
    with pytest.raises(ValueError):
        NH.gaussian2volume(SimpleNamespace(), None, {}, None, resolution=8, mode="points")
    if not torch.cuda.is_available():
        from nlosgr import GaussianParams
        model = GaussianParams.synthetic(8, 1, preset="torch", seed=1)
        kw = {"volume_position": torch.tensor([0.0, 0.5, 0.0]), "volume_size": 0.5}
        with pytest.raises(RuntimeError, match="GPU"):
            NH.gaussian2volume(SimpleNamespace(), model, kw, torch.zeros(3), resolution=4, mode="isosurface")
