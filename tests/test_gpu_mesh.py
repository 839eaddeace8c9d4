"""GPU tests of the surface output (nlosgr.mesh -> nlosgr_mesh_count / nlosgr_mesh_emit) against the CPU
oracle (tests/mesh_oracle.py, float64 on the same fp32 numbers: every case downloads the volume it uploaded).

The index topology (vertex count and order, faces) must be equal exactly.  Positions:
|hip - oracle| <= 2e-5 * (largest cell body diagonal) + 1e-6 * max|coordinate| -- a handful of fp32 roundings
of t and of the interpolation; values: the same with the largest value step along a crossing edge and
max|value|; normals: 1e-4 wherever the oracle's interpolated gradient is >= 1e-4 of the largest grid gradient
(normalising a tiny vector is ill-conditioned; the share left out must be <= 1 %)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mesh_oracle as MO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _grid(tabs):
    from nlosgr.voxelize import VoxelGrid
    return VoxelGrid(tables=[torch.from_numpy(np.ascontiguousarray(t)) for t in tabs])


def _hip(f, tabs, level, a=None):
    """(mesh as numpy arrays, the downloaded volume, the downloaded values volume)."""
    from nlosgr.mesh import isosurface
    vol = torch.from_numpy(f).to(DEV)
    val = torch.from_numpy(a).to(DEV) if a is not None else None
    m = isosurface(vol, _grid(tabs), level, values=val)
    assert m.vertices.dtype == torch.float32 and m.normals.dtype == torch.float32 and m.faces.dtype == torch.int32
    assert m.vertices.is_cuda and m.faces.is_cuda and m.normals.shape == m.vertices.shape
    out = SimpleNamespace(vertices=m.vertices.cpu().numpy(), normals=m.normals.cpu().numpy(),
                          values=None if m.values is None else m.values.cpu().numpy(), faces=m.faces.cpu().numpy())
    return out, vol.cpu().numpy(), None if val is None else val.cpu().numpy()


def _compare(got, ref, tabs, a, tag, normals=False):
    assert got.vertices.shape[0] == ref["vertices"].shape[0], tag
    assert got.faces.shape == ref["faces"].shape and np.array_equal(got.faces, ref["faces"]), tag
    diag = np.sqrt(sum(float(np.diff(t.astype(np.float64)).max()) ** 2 for t in tabs))
    cmax = max(float(np.abs(t).max()) for t in tabs)
    bound = 2e-5 * diag + 1e-6 * cmax
    err = np.abs(got.vertices.astype(np.float64) - ref["vertices"]).max()
    print(f"{tag}: {got.vertices.shape[0]} vertices, {got.faces.shape[0]} triangles; position err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, tag
    if a is not None:
        oi = np.stack(np.unravel_index(ref["owner"], a.shape), axis=1)
        fi = oi + np.asarray(MO.EDGE_DIRS)[ref["d"]]
        step = np.abs(a.astype(np.float64)[tuple(fi.T)] - a.astype(np.float64)[tuple(oi.T)]).max()
        vbound = 2e-5 * step + 1e-6 * float(np.abs(a).max())
        verr = np.abs(got.values.astype(np.float64) - ref["values"]).max()
        print(f"{tag}: value err {verr:.3e} (bound {vbound:.3e})")
        assert verr <= vbound, tag
    if normals:
        keep = ref["gnorm"] >= 1e-4 * ref["gmax"]
        share = 1.0 - keep.mean()
        nerr = np.abs(got.normals.astype(np.float64) - ref["normals"])[keep].max()
        print(f"{tag}: normals left out {100 * share:.4f} %, err {nerr:.3e}")
        assert share <= 0.01 and nerr <= 1e-4, tag
    return bound


@pytest.fixture(scope="module")
def noise():
    f, a, tabs = MO.noise_case()
    got, vol, val = _hip(f, tabs, 0.0, a)
    return SimpleNamespace(got=got, vol=vol, val=val, tabs=tabs, ref=MO.extract(vol, tabs, 0.0, val))


def test_noise_all_configurations(noise):
    """standard_normal seed 0, 9x17x70 (z > 64 crosses a wave's lane tile; odd extents leave partial tiles on
    every axis; the 10 710 points span eleven scan blocks), level 0, three different spacings.  From the oracle
    alone: all 256 corner configurations occur."""
    hist = MO.corner_configurations(noise.vol, 0.0)
    print(f"rarest corner configuration: {hist.min()} cells")
    assert (hist > 0).all()
    assert noise.ref["vertices"].shape[0] == 33556 and noise.ref["faces"].shape[0] == 66150
    _compare(noise.got, noise.ref, noise.tabs, noise.val, "noise", normals=False)
    assert np.isfinite(noise.got.normals).all()
    ln = np.linalg.norm(noise.got.normals.astype(np.float64), axis=1)
    assert (np.abs(ln - 1.0) <= 1e-6)[noise.ref["gnorm"] > 0].all()


def test_repeatable(noise):
    """Two runs of the noise case are bitwise equal in all four outputs."""
    f, a, tabs = MO.noise_case()
    again, _, _ = _hip(f, tabs, 0.0, a)
    for k in ("vertices", "normals", "values", "faces"):
        assert getattr(again, k).tobytes() == getattr(noise.got, k).tobytes(), k


@pytest.mark.parametrize("level", [0.3, 0.02])
def test_smooth_blobs(level):
    """Three anisotropic analytic Gaussians on 24x20x28 over the hidden-volume box: positions, values, normals,
    and the mesh is closed with the oracle's Euler characteristic and signed volume.  Share of vertices left
    out of the normal check, from the oracle alone on the CPU: 0 % at both levels."""
    f, a, tabs = MO.blobs_case()
    got, vol, val = _hip(f, tabs, level, a)
    ref = MO.extract(vol, tabs, level, val)
    bound = _compare(got, ref, tabs, val, f"blobs {level}", normals=True)
    assert MO.is_edge_manifold(got.faces) and MO.boundary_edges(got.faces).shape[0] == 0
    assert MO.euler_characteristic(got.faces) == MO.euler_characteristic(ref["faces"]) == 2
    v_got, v_ref = MO.signed_volume(got.vertices, got.faces), MO.signed_volume(ref["vertices"], ref["faces"])
    print(f"blobs {level}: signed volume {v_got:.8e} (oracle {v_ref:.8e})")
    # every vertex within `bound` of the oracle's: the enclosed volume moves by at most area x bound
    assert v_ref > 0 and abs(v_got - v_ref) <= MO.triangle_areas(ref["vertices"], ref["faces"]).sum() * bound
    assert MO.unreferenced_vertices(got.vertices.shape[0], got.faces) == 0


def test_exact_hits():
    """Integer-valued 7x6x5 volume at level 2: faces equal, every vertex finite, and a vertex on a corner hit
    (t = 0: the owner, t = 1: the far end) is that corner's coordinate exactly."""
    f, tabs = MO.exact_case()
    got, vol, _ = _hip(f, tabs, 2.0)
    ref = MO.extract(vol, tabs, 2.0)
    _compare(got, ref, tabs, None, "exact hits")
    assert np.isfinite(got.vertices).all() and np.isfinite(got.normals).all()
    oi = np.stack(np.unravel_index(ref["owner"], vol.shape), axis=1)
    fi = oi + np.asarray(MO.EDGE_DIRS)[ref["d"]]
    corner = lambda idx: np.stack([tabs[ax][idx[:, ax]] for ax in range(3)], axis=1)
    at0, at1 = ref["t"] == 0.0, ref["t"] == 1.0
    print(f"exact hits: {int(at0.sum())} vertices at t = 0, {int(at1.sum())} at t = 1 of {at0.size}")
    assert at0.sum() > 50 and at1.sum() > 50
    assert np.array_equal(got.vertices[at0], corner(oi)[at0])
    assert np.array_equal(got.vertices[at1], corner(fi)[at1])
    assert (MO.triangle_areas(got.vertices, got.faces) == 0).sum() == 346


def test_non_finite_voxels():
    """The blobs volume with one NaN, one +inf and one -inf voxel on the surface's path: they count as outside,
    the faces equal the oracle's and every output is finite."""
    f, a, tabs = MO.blobs_case()
    f = f.copy()
    clean = MO.extract(f, tabs, 0.3)
    oi = np.stack(np.unravel_index(clean["owner"], f.shape), axis=1)
    oi = oi[f[tuple(oi.T)] >= 0.3]               # inside voxels next to the surface: each one changes the faces
    picks = [tuple(oi[i]) for i in (len(oi) // 5, len(oi) // 2, 4 * len(oi) // 5)]
    assert len(set(picks)) == 3
    for p, v in zip(picks, (np.nan, np.inf, -np.inf)):
        f[p] = v
    got, vol, val = _hip(f, tabs, 0.3, a)
    ref = MO.extract(vol, tabs, 0.3, val)
    assert not np.array_equal(ref["faces"], clean["faces"])
    assert np.array_equal(got.faces, ref["faces"]) and got.vertices.shape[0] == ref["vertices"].shape[0]
    assert np.isfinite(got.vertices).all() and np.isfinite(got.normals).all() and np.isfinite(got.values).all()
    assert (ref["t"] == 0.5).sum() >= 3          # the edges that end in a non-finite voxel
    _compare(got, ref, tabs, val, "non-finite")


@pytest.mark.parametrize("case", ["thin", "outside", "inside", "nan"])
def test_degenerate_and_empty(case):
    """An extent < 2, an all-outside, an all-inside and an all-NaN volume: (0, 0) and empty tensors."""
    shape = (1, 5, 5) if case == "thin" else (5, 6, 7)
    f = np.random.default_rng(3).random(shape).astype(np.float32)
    if case == "nan":
        f[:] = np.nan
    level = {"thin": 0.5, "outside": 2.0, "inside": -1.0, "nan": 0.0}[case]
    tabs = MO.linspace_tables([(0.0, 1.0, n) for n in shape])
    got, _, val = _hip(f, tabs, level, f)
    assert got.vertices.shape == (0, 3) and got.normals.shape == (0, 3) and got.faces.shape == (0, 3)
    assert got.values.shape == (0,)
    assert MO.extract(f, tabs, level)["faces"].shape == (0, 3)


def test_wrong_counts_write_nothing():
    """nlosgr_mesh_emit with counts that disagree with the workspace's totals leaves the outputs untouched."""
    from nlosgr import _lib
    lib = _lib.load()
    f, tabs = MO.exact_case()
    vol = torch.from_numpy(f).to(DEV)
    grid = _grid(tabs)
    xs, ys, zs = grid.on(vol.device)
    vg = _lib.VoxelGrid(*f.shape, _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(zs))
    ws = torch.empty(lib.nlosgr_mesh_workspace_bytes(vg), dtype=torch.uint8, device=DEV)
    counts = torch.empty(2, dtype=torch.int64, device=DEV)
    stream = _lib.stream_handle(vol.device)
    _lib.check(lib.nlosgr_mesh_count(_lib.ptr(vol), vg, 2.0, _lib.ptr(ws), _lib.ptr(counts), stream))
    nv, nt = (int(c) for c in counts.cpu())
    ref = MO.extract(f, tabs, 2.0)
    assert (nv, nt) == (ref["vertices"].shape[0], ref["faces"].shape[0])
    for dv, dt in ((-1, 0), (0, -1), (1, 1)):
        verts = torch.full((nv + 1, 3), -7.0, device=DEV)
        tris = torch.full((nt + 1, 3), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.nlosgr_mesh_emit(_lib.ptr(vol), None, vg, 2.0, _lib.ptr(ws), nv + dv, nt + dt, _lib.ptr(verts),
                                        None, None, _lib.ptr(tris), stream))
        assert (verts == -7.0).all() and (tris == -7).all(), (dv, dt)
    verts = torch.full((nv + 1, 3), -7.0, device=DEV)
    tris = torch.full((nt + 1, 3), -7, dtype=torch.int32, device=DEV)
    _lib.check(lib.nlosgr_mesh_emit(_lib.ptr(vol), None, vg, 2.0, _lib.ptr(ws), nv, nt, _lib.ptr(verts), None, None,
                                    _lib.ptr(tris), stream))      # the right counts, no normals wanted
    assert np.array_equal(tris[:nt].cpu().numpy(), ref["faces"]) and (tris[nt] == -7).all() and (verts[nv] == -7.0).all()
    assert (verts[:nv] != -7.0).any(dim=1).all()


def test_end_to_end(tmp_path):
    """extract_mesh == isosurface of the voxelize output at the mean level; python -m nlosgr.mesh (its main(),
    in process) writes a PLY holding the same arrays; gaussian2volume(mode='isosurface') returns the same mesh."""
    from nlosgr import GaussianParams
    from nlosgr import nlos_helpers as NH
    from nlosgr.checkpoint import save_checkpoint
    from nlosgr.mesh import extract_mesh, isosurface, main, read_ply
    from nlosgr.voxelize import VoxelGrid, voxelize
    model = GaussianParams.synthetic(200, 2, preset="cuda", device=DEV, seed=6)
    pos, size = (0.02, 0.5, 0.0), 0.4
    grid = VoxelGrid(pos, size, 24)
    cam = torch.tensor((0.02, 0.0, 0.0), dtype=torch.float32, device=DEV)
    dens, alb = voxelize(model, grid, cam, preset="cuda", cutoff=3.0)
    level = dens.mean().item()
    want = isosurface(dens, grid, level, values=alb)
    assert want.vertices.shape[0] > 100 and want.faces.shape[0] > 100
    ref = MO.extract(dens.cpu().numpy(), [t.numpy() for t in grid.tables], level, alb.cpu().numpy())
    assert np.array_equal(want.faces.cpu().numpy(), ref["faces"])

    def same(m):
        return all(torch.equal(torch.as_tensor(x).to(DEV), y) for x, y in
                   ((m.vertices, want.vertices), (m.normals, want.normals), (m.values, want.values), (m.faces, want.faces)))

    got, used = extract_mesh(model, grid, cam, preset="cuda", cutoff=3.0)
    assert used == level and same(got)
    frac, used = extract_mesh(model, grid, cam, level_frac=0.25, field="albedo", preset="cuda", cutoff=3.0)
    assert used == 0.25 * alb.max().item()
    assert torch.equal(frac.faces, isosurface(alb, grid, used, values=dens).faces)

    ck, out = str(tmp_path / "model.pth"), str(tmp_path / "mesh.ply")
    save_checkpoint(ck, model)
    main([ck, "--resolution", "24", "--cutoff", "3", "--volume-position", "0.02", "0.5", "0", "--volume-size", "0.4",
          "--preset", "cuda", "--out", out])
    assert same(read_ply(out))

    args = SimpleNamespace(scaling_modifier=1.0, occlusion=False, use_cuda_renderer=True, render_cutoff=3.0)
    kw = {"volume_position": pos, "volume_size": size}
    res = NH.gaussian2volume(args, model, kw, cam, resolution=24, mode="isosurface")
    assert NH.CUDA_RENDERER is not None and torch.equal(res["density"], dens)
    assert res["level"] == level and same(res["mesh"])
    assert set(NH.gaussian2volume(args, model, kw, cam, resolution=24, mode="voxel")) == set(res) - {"mesh", "level"}
