"""CPU-only checks of the voxelizer's backward and the voxel-domain fit: the two exported symbols and their host
validation, the float64 gradient oracle (tests/voxel_grad_oracle.py) against central finite differences, and the
argument checks of nlosgr.voxel_fit and nlosgr.forward_project.project.  No GPU is touched."""
import ctypes

import pytest
import torch

import voxel_grad_oracle as GO
import voxel_oracle as VO


def test_symbols_are_exported_and_the_abi_stays_13():
    from nlosgr import _lib
    lib = _lib.load()
    for name in ("nlosgr_voxel_bwd_workspace_bytes", "nlosgr_voxelize_bwd"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.nlosgr_abi_version() == 13 and _lib.ABI_VERSION == 13


def test_backward_entry_points_validate_on_the_host():
    """Validation runs on the host before any launch and reports through nlosgr_last_error (fake non-null pointers
    are never read): validate_voxel's errors, plus a null cam, null outputs and a null workspace when ng > 0."""
    from nlosgr import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    G = lambda ng=10, p=fake: _lib.Gaussians(ng, 16, 3, _lib.PRESET_CUDA, 1.0, p, p, p, p, p)
    V = lambda nx=8, ny=8, nz=8, p=fake: _lib.VoxelGrid(nx, ny, nz, p, p, p)
    O = lambda mode=0, cutoff=3.0, cache=0, sel=0: _lib.Options(mode, cutoff, 0.0, 1.0, 0, 0, cache, sel, 0, 0)
    size = lib.nlosgr_voxel_bwd_workspace_bytes

    def bwd(g, v, o, cam=fake, ws=fake, outs=(fake,) * 5):
        return lib.nlosgr_voxelize_bwd(g, v, cam, o, ws, fake, fake, *outs, None)

    assert size(G(), V(), O()) > 0 and size(G(), V(), O(cutoff=0.0)) > 0
    assert size(G(1000), V(), O()) > size(G(10), V(), O())
    assert size(G(0), V(), O()) > 0                                      # the empty problem is a valid one
    assert bwd(G(0), V(), O(), ws=None, outs=(None,) * 5) == 0           # ng == 0: nothing to write
    # null structs and pointers
    assert size(None, V(), O()) == 0 and b"null" in lib.nlosgr_last_error()
    assert bwd(None, V(), O()) == 1 and bwd(G(), None, O()) == 1 and bwd(G(), V(), None) == 1
    assert bwd(G(p=None), V(), O()) == 1 and b"Gaussian parameter" in lib.nlosgr_last_error()
    assert size(G(p=None), V(), O()) == 0
    assert bwd(G(), V(p=None), O()) == 1 and b"table" in lib.nlosgr_last_error()
    assert size(G(), V(p=None), O()) == 0
    assert bwd(G(), V(), O(), cam=None) == 1 and b"camera" in lib.nlosgr_last_error()
    assert bwd(G(), V(), O(), ws=None) == 1 and b"workspace" in lib.nlosgr_last_error()
    for i in range(5):
        outs = tuple(None if j == i else fake for j in range(5))
        assert bwd(G(), V(), O(), outs=outs) == 1 and b"gradient output" in lib.nlosgr_last_error(), i
    # extents and options, as nlosgr_voxelize
    for bad in (dict(nx=0), dict(ny=0), dict(nz=0), dict(nx=1025), dict(ny=-3), dict(nz=4096)):
        assert bwd(G(), V(**bad), O()) == 1 and b"1..1024" in lib.nlosgr_last_error(), bad
        assert size(G(), V(**bad), O()) == 0
    for bad in (O(mode=_lib.MODE_NETF), O(mode=_lib.MODE_OCCL), O(cache=1), O(sel=_lib.SELECT_AABB)):
        assert bwd(G(), V(), bad) == 1 and b"cutoff only" in lib.nlosgr_last_error()
        assert size(G(), V(), bad) == 0
    g = _lib.Gaussians(10, 16, 4, _lib.PRESET_CUDA, 1.0, fake, fake, fake, fake, fake)
    assert bwd(g, V(), O()) == 3 and b"cuda preset" in lib.nlosgr_last_error() and size(g, V(), O()) == 0
    g = _lib.Gaussians(10, 9, 3, _lib.PRESET_TORCH, 1.0, fake, fake, fake, fake, fake)
    assert bwd(g, V(), O()) == 1 and b"k_feat" in lib.nlosgr_last_error()
    g = _lib.Gaussians(-1, 16, 3, _lib.PRESET_CUDA, 1.0, fake, fake, fake, fake, fake)
    assert bwd(g, V(), O()) == 1 and b"ng" in lib.nlosgr_last_error()


@pytest.mark.parametrize("preset", ["torch", "cuda"])
@pytest.mark.parametrize("mc", [None, 3.0])
def test_oracle_gradients_match_central_differences(preset, mc):
    """Pins the oracle itself: 6 Gaussians (the last with 0.5 + SH < 0: the clamp is active) x 5x4x6 voxels, both
    upstreams, every parameter entry by central differences in float64 (h = 1e-6; the cutoff case keeps every pair's
    m^2 away from the mask's edge by construction of the check below)."""
    g = torch.Generator().manual_seed(11)
    n, K = 6, 16
    p = dict(mu=torch.rand(n, 3, generator=g) * 0.3 + torch.tensor([-0.15, 0.4, -0.15]),
             scaling=(torch.randn(n, 3, generator=g) * 0.2 + (-2.2 if preset == "cuda" else -1.0)),
             rotation=torch.randn(n, 4, generator=g), opacity=torch.randn(n, 1, generator=g),
             features_dc=torch.rand(n, 1, 1, generator=g) * -1.0, features_rest=0.05 * torch.randn(n, K - 1, 1, generator=g))
    p["features_dc"][-1] = -3.0
    coords = VO.grid_coords(((-0.2, 0.2, 5), (0.4, 0.6, 4), (-0.2, 0.2, 6)))
    cam = (0.03, 0.0, -0.06)
    gd = torch.randn(5, 4, 6, generator=g).double()
    ga = torch.randn(5, 4, 6, generator=g).double()
    P = GO.params64(p, 3)
    if mc is not None:
        m2 = -2.0 * torch.log(GO.R.gaussian_pdf(coords.reshape(-1, 3).double(), P, preset, 1.0, None).detach())
        assert ((m2 - mc * mc).abs() > 1e-3).all() and (m2 <= mc * mc).any()
        assert preset == "torch" or (m2 > mc * mc).any()      # (torch preset: every std >= 1, nothing is cut)
    grads, scale = GO.reference(P, coords, cam, preset, gd, ga, mc=mc)
    assert GO.R.albedo(P, torch.tensor(cam).double(), preset)[-1].item() == 0.0
    assert (grads["features"][-1] == 0).all() and grads["features"][:-1].abs().max() > 0

    def L():
        with torch.no_grad():
            d, a = GO.volumes64(P, coords, cam, preset, 1.0, mc)
            return ((gd * d).sum() + (ga * a).sum()).item()

    h = 1e-6
    named = dict(mu="_mu", scaling="_scaling", rotation="_rotation", opacity="_opacity")
    for name, attr in named.items():
        t = getattr(P, attr)
        fd = torch.zeros_like(t)
        with torch.no_grad():
            for idx in range(t.numel()):
                old = t.view(-1)[idx].item()
                t.view(-1)[idx] = old + h
                up = L()
                t.view(-1)[idx] = old - h
                dn = L()
                t.view(-1)[idx] = old
                fd.view(-1)[idx] = (up - dn) / (2 * h)
        ref = grads[name].reshape(t.shape)
        err = (fd - ref).abs().max().item()
        assert err <= 1e-6 * ref.abs().max().item() + 1e-9, (name, err, ref.abs().max().item())
    # features: dc and two higher coefficients of every Gaussian
    for attr, cols, off in (("_features_dc", (0,), 0), ("_features_rest", (0, 9), 1)):
        t = getattr(P, attr)
        for gi in range(n):
            for c in cols:
                with torch.no_grad():
                    old = t[gi, c, 0].item()
                    t[gi, c, 0] = old + h
                    up = L()
                    t[gi, c, 0] = old - h
                    dn = L()
                    t[gi, c, 0] = old
                ref = grads["features"][gi, c + off].item()
                assert abs((up - dn) / (2 * h) - ref) <= 1e-6 * grads["features"].abs().max().item() + 1e-9, (attr, gi, c)
    # the scale bounds the gradient and is the sum of the two signed parts
    for nme in GO.NAMES:
        assert (grads[nme].abs().amax(dim=1) <= scale[nme] * (1 + 1e-12) + 1e-300).all(), nme


def test_voxel_fit_validates_its_arguments():
    from nlosgr.voxel_fit import VoxelFitStep
    from nlosgr.voxelize import VoxelGrid
    grid = VoxelGrid((0.0, 0.5, 0.0), 0.5, 4)
    rows = dict(rows=torch.zeros(2, 8), walls=torch.zeros(2, 3), r0=0.1, dr=0.01)
    with pytest.raises(ValueError, match="none was given"):
        VoxelFitStep(None, grid, (0, 0, 0))
    with pytest.raises(ValueError, match="both were given"):
        VoxelFitStep(None, grid, (0, 0, 0), target_volume=torch.zeros(4, 4, 4), **rows)
    for power in (-4, -1, 5):
        with pytest.raises(ValueError, match="0..4"):
            VoxelFitStep(None, grid, (0, 0, 0), power=power, **rows)
    with pytest.raises(ValueError, match="loss must be"):
        VoxelFitStep(None, grid, (0, 0, 0), loss="huber", **rows)
    with pytest.raises(TypeError):
        VoxelFitStep(None, None, (0, 0, 0), **rows)


def test_project_refuses_a_negative_power_with_grad():
    """The check comes before any GPU work: a volume that requires grad takes powers 0..4 only, and the message
    says why."""
    from nlosgr.forward_project import project
    from nlosgr.voxelize import VoxelGrid
    grid = VoxelGrid((0.0, 0.5, 0.0), 0.5, 4)
    vol = torch.zeros(4, 4, 4, requires_grad=True)
    for power in (-4, -1, 5):
        with pytest.raises(ValueError, match="backproject"):
            project(vol, torch.zeros(2, 3), grid, 0.1, 0.01, 8, power=power)


def test_command_line_parsing():
    from nlosgr.voxel_fit import parse_args
    a = parse_args(["cap.mat", "--resolution", "32", "--start", "100", "--end", "356", "--gaussians", "5000",
                    "--iterations", "200", "--power", "2", "--falloff", "2", "--cutoff", "4.5", "--out", "fit.pth",
                    "--recon", "recon.npz"])
    assert (a.capture, a.resolution, a.start, a.end, a.gaussians, a.iterations) == ("cap.mat", 32, 100, 356, 5000, 200)
    assert (a.power, a.falloff, a.cutoff, a.out, a.recon) == (2, 2.0, 4.5, "fit.pth", "recon.npz")
    d = parse_args(["cap.mat", "--start", "0", "--end", "8", "--gaussians", "1", "--iterations", "1", "--out", "o.pth"])
    assert (d.power, d.falloff, d.cutoff, d.recon, d.loss) == (0, 0.0, 3.0, None, "mse")
    for bad in (["--start", "8", "--end", "8"], ["--start", "0", "--end", "8", "--power", "-1"],
                ["--start", "0", "--end", "8", "--power", "5"], ["--start", "0", "--end", "8", "--iterations", "0"],
                ["--start", "0", "--end", "8", "--gaussians", "0"]):
        argv = ["cap.mat", "--gaussians", "4", "--iterations", "2", "--out", "o.pth"] + bad
        with pytest.raises(SystemExit):
            parse_args(argv)
