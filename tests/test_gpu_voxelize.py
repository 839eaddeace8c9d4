"""GPU tests of the reconstruction output (nlosgr.voxelize -> nlosgr_voxelize / nlosgr_volume_project)
against the reference's fixture, the CPU oracle (tests/voxel_oracle.py, float64) and itself.
Forward tolerance: max|hip - ref| <= 2e-5 * max|ref| + 1e-7 (tests/test_gpu_parity.py:14-23)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_case

import voxel_oracle as VO

pytestmark = pytest.mark.gpu

FWD_RTOL = 2e-5
DEV = "cuda:0"


def _close(a, b, rtol=FWD_RTOL, atol=1e-7, msg="", keep=None):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max()
    diff = np.abs(a - b)
    if keep is not None:
        diff = diff[np.asarray(keep)]
    err = diff.max()
    print(f"{msg}: max err {err:.3e} vs scale {scale:.3e} (ratio {err / scale:.2e})")
    assert err <= rtol * scale + atol, f"{msg}: max err {err:.3e} vs scale {scale:.3e}"


def _model(p, deg, dev=DEV):
    from nlosgr import GaussianParams
    t = lambda k: torch.as_tensor(p[k]).float().to(dev).contiguous()
    return GaussianParams(t("mu"), t("scaling"), t("rotation"), t("opacity"), t("features_dc"), t("features_rest"),
                          deg, deg)


def _cam(c=VO.PARITY_CAM):
    return torch.tensor(c, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("deg", [3, 4])
@pytest.mark.parametrize("mod", [1.0, 0.7])
def test_fixture_parity(deg, mod):
    """Torch preset, dense, on the reference's 6x5x7 grid (one partial brick: every edge mask) against
    estimate_rho_w_no_occlusion(out_separately=True) of the reference itself."""
    from nlosgr.voxelize import VoxelGrid, voxelize
    d = load_case("voxel_g32")
    p = {k: d[f"d{deg}_{k}"] for k in ("mu", "scaling", "rotation", "opacity", "features_dc", "features_rest")}
    grid = VoxelGrid(tables=[torch.from_numpy(d[k]) for k in ("xs", "ys", "zs")])
    dens, alb = voxelize(_model(p, deg), grid, _cam(d["cam"]), preset="torch", cutoff=0.0, scaling_modifier=mod)
    tag = f"d{deg}_m{str(mod).replace('.', 'p')}"
    assert dens.shape == (6, 5, 7) and alb.shape == (6, 5, 7)
    _close(dens.cpu(), d[tag + "_density"], msg=tag + " density")
    _close(alb.cpu(), d[tag + "_rho_density"], msg=tag + " rho_density")
    only_d, none_a = voxelize(_model(p, deg), grid, _cam(d["cam"]), preset="torch", cutoff=0.0,
                              scaling_modifier=mod, want_albedo=False)
    assert none_a is None and torch.equal(only_d, dens)


@pytest.fixture(scope="module")
def parity():
    """The 150-Gaussian / 40x9x33 problem of voxel_oracle.py: models on the GPU and the float64 oracle
    volumes per (preset, cutoff), computed once."""
    from nlosgr.voxelize import VoxelGrid
    grid = VoxelGrid(axes=VO.parity_axes())
    out = {"grid": grid}
    for preset in ("torch", "cuda"):
        p = VO.parity_gaussians(preset)
        out[preset] = {"p": p, "model": _model(p, 3)}
        P = VO.params_of(p, 3, double=True)
        for mc in (0.0, 3.0, 5.7):
            out[preset][mc] = VO.volumes(P, grid.coords(), VO.PARITY_CAM, preset, 1.0, mc if mc > 0 else None)
    return out


@pytest.mark.parametrize("preset", ["torch", "cuda"])
@pytest.mark.parametrize("cutoff", [0.0, 3.0, 5.7])
def test_oracle_parity(parity, preset, cutoff):
    """Both presets at cutoff 0 / 3 / 5.7 on 40x9x33 voxels (no extent a brick multiple, two super-bricks in
    x and z) with 150 Gaussians (three hit words, the last one partial), five of them hand-placed
    (voxel_oracle.parity_gaussians).  The support mask is discontinuous, so voxels for which some
    Gaussian's float64 m^2 lies within 1e-4 cutoff^2 of cutoff^2 are left out; that share must stay
    <= 0.5 %.  Measured with the oracle alone at seed 5: cuda preset 0.0000 % (cutoff 3) and 0.0842 %
    (cutoff 5.7); torch preset 0 % (every std >= 1: no voxel is near a support boundary)."""
    from nlosgr.voxelize import voxelize
    ref_d, ref_a, near = parity[preset][cutoff]
    share = near.float().mean().item()
    print(f"{preset} cutoff {cutoff}: excluded share {100 * share:.4f} %")
    assert share <= 0.005
    dens, alb = voxelize(parity[preset]["model"], parity["grid"], _cam(), preset=preset, cutoff=cutoff)
    keep = ~near.numpy()
    _close(dens.cpu(), ref_d, msg=f"{preset} {cutoff} density", keep=keep)
    _close(alb.cpu(), ref_a, msg=f"{preset} {cutoff} albedo", keep=keep)


def test_repeatable_and_independent_of_bricks(parity):
    """Cutoff 3: two runs are bitwise equal, and a sub-grid (offsets that are no brick multiples, so every
    voxel lands in another brick, lane and super-brick) gives exactly the full grid's numbers — the check
    on binning and compaction order."""
    from nlosgr.voxelize import voxelize
    grid, model = parity["grid"], parity["cuda"]["model"]
    dens, alb = voxelize(model, grid, _cam(), preset="cuda", cutoff=3.0)
    dens2, alb2 = voxelize(model, grid, _cam(), preset="cuda", cutoff=3.0)
    assert torch.equal(dens, dens2) and torch.equal(alb, alb2)
    assert (dens > 0).all()      # the grid-covering Gaussian reaches every voxel
    for ix, iy, iz in (((3, 29), (1, 8), (5, 31)), ((13, 40), (0, 9), (17, 33)), ((31, 34), (2, 3), (30, 33))):
        sd, sa = voxelize(model, grid.slice(ix, iy, iz), _cam(), preset="cuda", cutoff=3.0)
        sl = (slice(*ix), slice(*iy), slice(*iz))
        assert torch.equal(sd, dens[sl]), (ix, iy, iz)
        assert torch.equal(sa, alb[sl]), (ix, iy, iz)


def test_nan_gaussian_is_skipped(parity):
    """A Gaussian with a NaN mu in the middle of the index range: at cutoff 3 the output is bitwise the
    output without it (its cutoff box is not finite, so the culling skips it, as the forward does)."""
    from nlosgr.voxelize import voxelize
    p = parity["cuda"]["p"]
    q = {}
    for k, v in p.items():
        row = v[75:76].clone()
        if k == "mu":
            row[0, 1] = float("nan")
        q[k] = torch.cat((v[:75], row, v[75:]), dim=0)
    want = voxelize(parity["cuda"]["model"], parity["grid"], _cam(), preset="cuda", cutoff=3.0)
    got = voxelize(_model(q, 3), parity["grid"], _cam(), preset="cuda", cutoff=3.0)
    assert q["mu"].shape[0] == 151 and torch.isnan(q["mu"][75, 1])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_culled_converges_to_dense_at_moderate_size():
    """20k synthetic Gaussians (cuda preset) onto 64^3 at cutoff 5.7 against the HIP dense evaluation of two
    sub-grids: rel-L2 <= 1e-4, the bound test_cutoff_converges_to_dense holds the renderer to at 5 sigma."""
    from nlosgr import GaussianParams
    from nlosgr.voxelize import VoxelGrid, voxelize
    model = GaussianParams.synthetic(20000, 3, preset="cuda", device=DEV, seed=3)
    grid = VoxelGrid((0.0, 0.5, 0.0), 0.5, 64)
    dens, alb = voxelize(model, grid, _cam(), preset="cuda", cutoff=5.7)
    for ix, iy, iz in (((5, 23), (30, 47), (9, 28)), ((40, 64), (0, 11), (47, 64))):
        dd, da = voxelize(model, grid.slice(ix, iy, iz), _cam(), preset="cuda", cutoff=0.0)
        sl = (slice(*ix), slice(*iy), slice(*iz))
        for got, ref, name in ((dens[sl], dd, "density"), (alb[sl], da, "albedo")):
            rel = ((got.double() - ref.double()).norm() / ref.double().norm()).item()
            print(f"{name} {ix} {iy} {iz}: rel-L2 {rel:.3e}")
            assert ref.abs().max().item() > 0 and rel <= 1e-4, (name, rel)


def test_projection_matches_numpy():
    """All three axes of a 19x70x5 volume holding an all-zero column, a column with a repeated maximum and
    a negative-only column (per axis), against numpy.max / numpy.argmax of the same downloaded array."""
    from nlosgr.voxelize import project
    g = torch.Generator().manual_seed(2)
    vol = torch.randn(19, 70, 5, generator=g)
    vol[3, :, 2] = 0.0
    vol[:, 10, 1] = 0.0
    vol[4, 6, :] = 0.0
    vol[7, :, 4] = -vol[7, :, 4].abs() - 0.1
    vol[:, 20, 3] = -vol[:, 20, 3].abs() - 0.1
    vol[9, 30, :] = -vol[9, 30, :].abs() - 0.1
    vol[5, 11, 0] = vol[5, 40, 0] = vol[5, 69, 0] = 9.0
    vol[2, 33, 2] = vol[17, 33, 2] = 9.0
    vol[12, 50, 1] = vol[12, 50, 3] = 9.0
    host = vol.to(DEV).cpu().numpy()
    for axis in (0, 1, 2):
        mx, am = project(vol.to(DEV), axis=axis)
        assert am.dtype == torch.int32
        assert np.array_equal(mx.cpu().numpy(), host.max(axis=axis)), axis
        assert np.array_equal(am.cpu().numpy(), host.argmax(axis=axis)), axis
    mx, am = project(vol.to(DEV))                      # default: along y
    assert (mx[3, 2].item(), am[3, 2].item()) == (0.0, 0) and am[5, 0].item() == 11
    assert mx[7, 4].item() < 0 and mx[7, 4].item() == host[7, :, 4].max()


def test_gaussian2volume_voxel_mode():
    """gaussian2volume('voxel') at resolution 16: front / depth are the y projection of the albedo volume
    and ys[argmax], consistent with density / albedo recomputed through voxelize and project."""
    from nlosgr import GaussianParams
    from nlosgr import nlos_helpers as NH
    from nlosgr.voxelize import project, voxelize
    model = GaussianParams.synthetic(64, 3, preset="torch", device=DEV, seed=4)
    args = SimpleNamespace(scaling_modifier=0.7, occlusion=False)
    data_kwargs = {"volume_position": torch.tensor([0.0, 0.5, 0.0], device=DEV), "volume_size": 0.5}
    cam = torch.tensor([0.0, 0.0, 0.0], device=DEV)
    out = NH.gaussian2volume(args, model, data_kwargs, cam, resolution=16, mode="voxel")
    grid = out["grid"]
    assert grid.shape == (16, 16, 16) and out["density"].shape == (16, 16, 16)
    assert np.array_equal(grid.ys.numpy(), np.linspace(0.25, 0.75, 16).astype(np.float32))
    dens, alb = voxelize(model, grid, cam, preset="torch", cutoff=0.0, scaling_modifier=0.7)
    assert torch.equal(out["density"], dens) and torch.equal(out["albedo"], alb)
    assert (dens > 0).all() and (alb <= dens).all()
    for vol, f, dp in ((alb, "front", "depth"), (dens, "front_density", "depth_density")):
        mx, am = project(vol, axis=1)
        assert torch.equal(out[f], mx) and torch.equal(out[f], vol.max(dim=1).values)
        assert torch.equal(out[dp], grid.ys.to(DEV)[am.long()])
        assert out[dp].shape == (16, 16) and out[dp].min() >= 0.25 and out[dp].max() <= 0.75


def test_command_line_writes_reconstruction(tmp_path):
    """python -m nlosgr.voxelize (its main(), in process): checkpoint -> recon.npz, camera defaulting to the
    volume position projected onto the wall."""
    from nlosgr import GaussianParams
    from nlosgr.checkpoint import save_checkpoint
    from nlosgr.voxelize import VoxelGrid, main, voxelize
    model = GaussianParams.synthetic(200, 2, preset="cuda", device=DEV, seed=6)
    ck, out = str(tmp_path / "model.pth"), str(tmp_path / "recon.npz")
    save_checkpoint(ck, model)
    main([ck, "--resolution", "12", "--cutoff", "3", "--volume-position", "0.02", "0.5", "0", "--volume-size", "0.4",
          "--preset", "cuda", "--out", out])
    z = np.load(out)
    assert z["density"].shape == (12, 12, 12) and z["front"].shape == (12, 12) and z["depth"].shape == (12, 12)
    assert np.array_equal(z["cam"], np.array([0.02, 0.0, 0.0], dtype=np.float32))
    dens, alb = voxelize(model, VoxelGrid((0.02, 0.5, 0.0), 0.4, 12), _cam((0.02, 0.0, 0.0)), preset="cuda", cutoff=3.0)
    assert np.array_equal(z["density"], dens.cpu().numpy()) and np.array_equal(z["albedo"], alb.cpu().numpy())
    assert np.array_equal(z["front"], z["albedo"].max(axis=1))
