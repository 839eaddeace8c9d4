"""CPU-only checks of the reconstruction output (nlosgr.voxelize): the oracle formula against the
reference's fixture, the grid tables, slicing, host-side validation of the three C entry points and the
mesh refusal.  No GPU is touched."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_case

import voxel_oracle as VO

FWD_RTOL = 2e-5   # of the array maximum (tests/test_gpu_parity.py:14-23)


def _close(a, b, rtol=FWD_RTOL, atol=1e-7, msg=""):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    err, scale = np.abs(a - b).max(), np.abs(b).max()
    assert err <= rtol * scale + atol, f"{msg}: max err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("deg", [3, 4])
@pytest.mark.parametrize("mod", [1.0, 0.7])
@pytest.mark.parametrize("double", [False, True])
def test_oracle_reproduces_reference_fixture(deg, mod, double):
    """sum_g sigma pdf and sum_g sigma rho pdf from oracle.torch_ref.gaussian_pdf / albedo equal what the
    reference's estimate_rho_w_no_occlusion(out_separately=True) returned on the 6x5x7 grid."""
    d = load_case("voxel_g32")
    p = {k: d[f"d{deg}_{k}"] for k in ("mu", "scaling", "rotation", "opacity", "features_dc", "features_rest")}
    coords = torch.stack(torch.meshgrid(*(torch.from_numpy(d[k]) for k in ("xs", "ys", "zs")), indexing="ij"), -1)
    dens, alb, _ = VO.volumes(VO.params_of(p, deg, double), coords, d["cam"], "torch", mod)
    tag = f"d{deg}_m{str(mod).replace('.', 'p')}"
    assert tuple(dens.shape) == (6, 5, 7)
    _close(dens, d[tag + "_density"], msg=tag + " density")
    _close(alb, d[tag + "_rho_density"], msg=tag + " rho_density")


def test_voxel_grid_tables_are_linspace_in_ij_order():
    from nlosgr.voxelize import VoxelGrid
    g = VoxelGrid((0.1, 0.5, -0.2), 0.5, (6, 5, 7))
    assert g.shape == (6, 5, 7)
    for t, c, n in zip(g.tables, (0.1, 0.5, -0.2), (6, 5, 7)):
        want = np.linspace(c - 0.25, c + 0.25, n).astype(np.float32)
        assert t.dtype == torch.float32 and np.array_equal(t.numpy(), want)
        assert t[0].item() == np.float32(c - 0.25) and t[-1].item() == np.float32(c + 0.25)   # end points included
        np.testing.assert_allclose(t.numpy(), torch.linspace(c - 0.25, c + 0.25, n).numpy(), rtol=1e-6, atol=1e-7)
    c = g.coords()
    assert c.shape == (6, 5, 7, 3)
    want = np.stack(np.meshgrid(*(t.numpy() for t in g.tables), indexing="ij"), -1)
    assert np.array_equal(c.numpy(), want)
    assert np.array_equal(c.reshape(-1, 3)[(2 * 5 + 3) * 7 + 4].numpy(), [g.xs[2], g.ys[3], g.zs[4]])
    e = VoxelGrid(axes=((0.0, 1.0, 3), (2.0, 3.0, 1), (-1.0, 1.0, 5)))
    assert e.shape == (3, 1, 5) and np.array_equal(e.zs.numpy(), np.linspace(-1, 1, 5).astype(np.float32))
    assert VoxelGrid((0, 0.5, 0), 0.5, 8).shape == (8, 8, 8)
    with pytest.raises(ValueError):
        VoxelGrid((0, 0.5, 0), 0.5, 1025)
    with pytest.raises(ValueError):
        VoxelGrid()


def test_voxel_grid_slice_shares_table_values():
    from nlosgr.voxelize import VoxelGrid
    g = VoxelGrid(axes=VO.parity_axes())
    s = g.slice(ix=(3, 29), iz=(5, 31))
    assert s.shape == (26, 9, 26)
    assert torch.equal(s.xs, g.xs[3:29]) and torch.equal(s.ys, g.ys) and torch.equal(s.zs, g.zs[5:31])
    assert s.xs.data_ptr() == g.xs[3:29].data_ptr()          # a view of the parent's table, not a new linspace
    assert torch.equal(s.coords(), g.coords()[3:29, :, 5:31])


def test_voxel_entry_points_validate_on_the_host():
    """Argument validation of nlosgr_voxel_workspace_bytes / nlosgr_voxelize / nlosgr_volume_project runs on
    the host and reports through nlosgr_last_error (no GPU, fake non-null pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    G = lambda ng=10, p=fake: _lib.Gaussians(ng, 16, 3, _lib.PRESET_CUDA, 1.0, p, p, p, p, p)
    V = lambda nx=8, ny=8, nz=8, p=fake: _lib.VoxelGrid(nx, ny, nz, p, p, p)
    O = lambda mode=0, cutoff=3.0, cache=0, sel=0: _lib.Options(mode, cutoff, 0.0, 1.0, 0, 0, cache, sel, 0, 0)
    vox = lambda g, v, o, cam=fake, ws=fake, d=fake, a=fake: lib.nlosgr_voxelize(g, v, cam, o, ws, d, a, None)

    assert lib.nlosgr_voxel_workspace_bytes(G(), V(), O()) > 0
    assert lib.nlosgr_voxel_workspace_bytes(G(), V(), O(cutoff=0.0)) > 0
    assert lib.nlosgr_voxel_workspace_bytes(G(), V(), O()) > lib.nlosgr_voxel_workspace_bytes(G(), V(), O(cutoff=0.0))
    assert lib.nlosgr_voxel_workspace_bytes(G(0), V(), O()) > 0          # empty problem is a valid one
    # null structs and pointers
    assert lib.nlosgr_voxel_workspace_bytes(None, V(), O()) == 0 and b"null" in lib.nlosgr_last_error()
    assert vox(None, V(), O()) == 1 and vox(G(), None, O()) == 1 and vox(G(), V(), None) == 1
    assert vox(G(p=None), V(), O()) == 1 and b"Gaussian parameter" in lib.nlosgr_last_error()
    assert vox(G(), V(p=None), O()) == 1 and b"table" in lib.nlosgr_last_error()
    assert vox(G(), V(), O(), cam=None) == 1 and b"camera" in lib.nlosgr_last_error()
    assert vox(G(), V(), O(), ws=None) == 1 and b"workspace" in lib.nlosgr_last_error()
    assert vox(G(), V(), O(), ws=None, d=None, a=None) == 0              # nothing asked for: nothing to do
    # extents
    for bad in (dict(nx=0), dict(ny=0), dict(nz=0), dict(nx=1025), dict(ny=-3), dict(nz=4096)):
        assert vox(G(), V(**bad), O()) == 1 and b"1..1024" in lib.nlosgr_last_error(), bad
        assert lib.nlosgr_voxel_workspace_bytes(G(), V(**bad), O()) == 0
    assert lib.nlosgr_voxel_workspace_bytes(G(), V(1024, 1, 1024), O()) > 0
    # only opt->cutoff is used
    for bad in (O(mode=_lib.MODE_NETF), O(mode=_lib.MODE_OCCL), O(cache=1), O(sel=_lib.SELECT_AABB)):
        assert vox(G(), V(), bad) == 1 and b"cutoff only" in lib.nlosgr_last_error()
        assert lib.nlosgr_voxel_workspace_bytes(G(), V(), bad) == 0
    # the Gaussian checks of the renderer
    g = _lib.Gaussians(10, 16, 4, _lib.PRESET_CUDA, 1.0, fake, fake, fake, fake, fake)
    assert vox(g, V(), O()) == 3 and b"cuda preset" in lib.nlosgr_last_error()
    g = _lib.Gaussians(10, 9, 3, _lib.PRESET_TORCH, 1.0, fake, fake, fake, fake, fake)
    assert vox(g, V(), O()) == 1 and b"k_feat" in lib.nlosgr_last_error()
    # projection
    proj = lambda vol=fake, nx=4, ny=5, nz=6, axis=1, mx=fake, am=fake: lib.nlosgr_volume_project(
        vol, nx, ny, nz, axis, mx, am, None)
    assert proj(vol=None) == 1 and b"null volume" in lib.nlosgr_last_error()
    assert proj(mx=None, am=None) == 1 and b"null projection" in lib.nlosgr_last_error()
    for axis in (-1, 3, 7):
        assert proj(axis=axis) == 1 and b"axis" in lib.nlosgr_last_error()
    for bad in (dict(nx=0), dict(ny=1025), dict(nz=-1)):
        assert proj(**bad) == 1 and b"1..1024" in lib.nlosgr_last_error()


def test_python_surface_refuses_cpu_tensors():
    """float32 GPU tensors only: anything else raises RuntimeError (as carve_votes does), no CPU fallback."""
    from nlosgr import GaussianParams
    from nlosgr.voxelize import VoxelGrid, project, voxelize
    model = GaussianParams.synthetic(8, 1, preset="cuda", seed=1)            # CPU tensors
    with pytest.raises(RuntimeError, match="GPU"):
        voxelize(model, VoxelGrid((0, 0.5, 0), 0.5, 4), torch.zeros(3))
    with pytest.raises(RuntimeError, match="GPU"):
        project(torch.zeros(3, 4, 5))


def test_gaussian2volume_mesh_mode_raises():
    from types import SimpleNamespace
    from nlosgr import nlos_helpers as NH
    with pytest.raises(NotImplementedError, match="open3d"):
        NH.gaussian2volume(SimpleNamespace(), None, {}, None, resolution=8, mode="mesh")
    with pytest.raises(ValueError):
        NH.gaussian2volume(SimpleNamespace(), None, {}, None, resolution=8, mode="points")
