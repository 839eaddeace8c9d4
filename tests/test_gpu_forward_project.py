"""GPU checks of the forward projection (include/nlosgr.h ABI 13, csrc/nlosgr_forward_project.hip) against the
float64 oracle of tests/forward_project_oracle.py: |gpu - oracle| <= B per bin, with B the oracle's derived bound
and no further factor.  `-s` prints the worst measured e/B per case.

Shapes are the smallest at which the kernel can go wrong: one voxel, grids whose size is no multiple of a lane's
run of 4 voxels or of a workgroup's step of 1024, a grid of several steps (the library then splits the voxels
over workgroups and finishes from the int64 workspace); one wall point, three (two per workgroup, the last
workgroup half empty) and 257 (four per workgroup, the last one holding a single wall point); rows of one, two
and three bins, a short row, a long one (1024 bins: four rows are exactly the 32 KiB a workgroup may hold) and
the longest allowed (8192 bins: one wall point per workgroup); r0 = 0 and > 0; every power.
The volume reaches in front of the window and behind it (the window ends at 0.9, the farthest voxel is 1.28 from
the farthest wall point) and voxel (0, 0, 0) sits on wall point 0 (d = 0)."""
import math

import numpy as np
import pytest
import torch

import backproject_oracle as BO
import forward_project_oracle as FO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRIDS = [(1, 1, 1), (9, 5, 13), (17, 8, 3), (16, 16, 16)]
WALLS = [1, 3, 257]
NRS = [1, 2, 3, 40, 1024]
R0S = [0.0, 0.3]
FAR = 0.9
CASES = [(g, nw, nr, r0) for g in GRIDS for nw in WALLS for nr in NRS for r0 in R0S] + [((9, 5, 13), 1, 8192, 0.3)]


def _tables(shape):
    nx, ny, nz = shape
    return (np.linspace(-0.3, 0.3, nx).astype(np.float32), np.linspace(0.0, 0.6, ny).astype(np.float32),
            np.linspace(-0.3, 0.3, nz).astype(np.float32))


def _walls(nwall, tabs, g):
    w = np.zeros((nwall, 3), dtype=np.float32)
    w[:, 0] = g.random(nwall) - 0.5
    w[:, 2] = g.random(nwall) - 0.5
    w[0] = (tabs[0][0], tabs[1][0], tabs[2][0])        # voxel (0, 0, 0) coincides with wall point 0
    return w


def _grid(tabs):
    from nlosgr.voxelize import VoxelGrid
    return VoxelGrid(tables=[torch.from_numpy(np.ascontiguousarray(t)) for t in tabs])


def _problem(shape, nwall, nr, r0, seed=0):
    g = np.random.default_rng(seed + 1000 * nwall + nr + sum(shape))
    tabs = _tables(shape)
    walls = _walls(nwall, tabs, g)
    vol = g.standard_normal(shape).astype(np.float32)
    dr = (FAR - r0) / nr
    return dict(shape=shape, nwall=nwall, nr=nr, r0=r0, dr=dr, tabs=tabs, walls=walls, vol=vol,
                d=BO.distances64(walls, *tabs))


def _powers(c):
    from nlosgr.backproject import fp32_window
    r0, inv_dr = fp32_window(c["r0"], c["dr"])
    return list(range(5)) + ([-1, -2, -3, -4] if r0 * inv_dr >= 2 else [])


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"g{'x'.join(map(str, p[0]))}-w{p[1]}-nr{p[2]}-r{p[3]}")
def case(request):
    return _problem(*request.param)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gpu(c, power=0, vol=None, grid=None, **kw):
    from nlosgr.forward_project import forward_project
    return forward_project(_dev(c["vol"] if vol is None else vol), _dev(c["walls"]), grid or _grid(c["tabs"]), c["r0"],
                           c["dr"], c["nr"], power=power, **kw)


def _oracle(c, power, vol=None, **kw):
    from nlosgr.backproject import fp32_window
    r0, inv_dr = fp32_window(c["r0"], c["dr"])
    return FO.forward64(c["vol"] if vol is None else vol, c["walls"], *c["tabs"], r0, inv_dr, c["nr"], power, d=c["d"],
                        **kw)


def _share(err, B):
    m = B > 0
    return float((err[m] / B[m]).max()) if m.any() else 0.0


def test_parity_within_the_bound(case):
    worst = []
    powers = _powers(case)
    for power in powers:
        ref, B = _oracle(case, power)
        got = _gpu(case, power).cpu().numpy().astype(np.float64)
        assert got.shape == (case["nwall"], case["nr"]) and np.isfinite(got).all()
        err = np.abs(got - ref)
        worst.append(_share(err, B))
        assert np.all(err <= B), (power, worst[-1])
    print(f"grid {case['shape']} walls {case['nwall']} nr {case['nr']} r0 {case['r0']}: worst e/B for powers "
          f"{powers[0]}..{powers[-1] if len(powers) == 5 else '4, -1..-4'}: " + " ".join(f"{w:.4f}" for w in worst))


def test_cases_reach_every_part_of_the_window():
    """The placement the parity cases rely on, checked once on the oracle's bin coordinate; a wrong bin or a
    wrong weight is far outside the bound."""
    from nlosgr.backproject import fp32_window
    c = _problem((9, 5, 13), 257, 40, 0.3)
    u = BO.bin_coordinate(c["d"], *fp32_window(c["r0"], c["dr"]))
    nr = c["nr"]
    assert (u <= -1).any() and ((u > -1) & (u < 0)).any() and ((u >= 0) & (u <= nr - 1)).any()
    assert ((u > nr - 1) & (u < nr)).any() and (u >= nr).any()
    assert c["d"][0, 0] == 0.0
    ref, B = _oracle(c, 2)
    assert (np.abs(np.roll(ref, 1, axis=1) - ref) > 100 * B).any()
    assert (np.abs(_oracle(c, 1, want_bound=False)[0] - ref) > 100 * B).any()


def test_repeatable_and_independent_of_the_split():
    """Two runs are bitwise equal, the forced splits 1, 2 and 7 equal the library's choice, and a volume that is
    zero outside a sub-grid gives bitwise the rows of the call on that sub-grid (same max|vol|; 17 x 10 x 21 and
    19 x 10 x 21 voxels share ceil(log2(2 nvox)) = 13, so the quantum is the same)."""
    c = _problem((19, 10, 21), 3, 40, 0.3)
    grid = _grid(c["tabs"])
    vol = c["vol"].copy()
    vol[:2] = 0.0
    assert np.abs(vol).max() == np.abs(vol[2:]).max()
    for power in (0, 3, -2):
        full = _gpu(c, power, grid=grid)
        assert full.any() and torch.equal(full, _gpu(c, power, grid=grid))
        for ns in (1, 2, 7):
            assert torch.equal(full, _gpu(c, power, grid=grid, nsplit=ns)), (power, ns)
        part = _gpu(c, power, vol=vol, grid=grid)
        for ns in (0, 1, 7):
            sub = _gpu(c, power, vol=vol[2:], grid=grid.slice(ix=(2, 19)), nsplit=ns)
            assert torch.equal(sub, part), (power, ns)
    many = _problem((16, 16, 16), 257, 40, 0.3)                    # one split against the library's 4 and a forced 7
    one = _gpu(many, 2, nsplit=1)
    assert torch.equal(one, _gpu(many, 2)) and torch.equal(one, _gpu(many, 2, nsplit=7))


def test_accumulate_and_overwrite():
    c = _problem((9, 5, 13), 257, 40, 0.3)
    grid = _grid(c["tabs"])
    lo, hi = grid.slice(ix=(0, 4)), grid.slice(ix=(4, 9))
    for power in (0, 2, -4):
        ref, B = _oracle(c, power)
        one = _gpu(c, power, grid=grid)
        acc = _gpu(c, power, vol=c["vol"][:4], grid=lo)
        same = _gpu(c, power, vol=c["vol"][4:], grid=hi, out=acc, accumulate=True)
        assert same is acc
        a, o = acc.cpu().numpy(), one.cpu().numpy()
        ulp = np.spacing(np.abs(o)).astype(np.float64)
        diff = np.abs(a.astype(np.float64) - o.astype(np.float64))
        print(f"accumulate power {power}: worst |halves - one| / (B + ulp) {float((diff / (B + ulp)).max()):.4f}")
        assert np.all(diff <= B + ulp)
        filled = torch.full((c["nwall"], c["nr"]), float("nan"), device=DEV)
        assert torch.equal(_gpu(c, power, grid=grid, out=filled), one) and torch.equal(filled, one)
    # no wall points: nothing is written
    from nlosgr.forward_project import forward_project
    empty = forward_project(_dev(c["vol"]), torch.zeros(0, 3, device=DEV), grid, 0.3, 0.015, 40)
    assert empty.shape == (0, 40)


@pytest.mark.parametrize("nsplit", [1, 2])
def test_edge_values(nsplit):
    """A zero volume gives zero rows; one NaN or one inf voxel makes every row NaN (with one split and through
    the workspace), also for a voxel no wall point's window reaches."""
    c = _problem((9, 5, 13), 3, 40, 0.3)
    zero = np.zeros(c["shape"], dtype=np.float32)
    out = torch.full((3, 40), 7.0, device=DEV)
    assert not _gpu(c, 0, vol=zero, out=out, nsplit=nsplit).any()
    kept = _gpu(c, 0, vol=zero, out=torch.full((3, 40), 7.0, device=DEV), accumulate=True, nsplit=nsplit)
    assert (kept == 7.0).all()
    for bad in (np.nan, np.inf, -np.inf):
        for at in ((4, 2, 6), (0, 0, 0), (8, 4, 12)):
            vol = c["vol"].copy()
            vol[at] = bad
            got = _gpu(c, 1, vol=vol, nsplit=nsplit)
            assert torch.isnan(got).all(), (bad, at)
    got = _gpu(c, 0, vol=np.where(np.arange(585).reshape(c["shape"]) == 77, np.nan, 0.0).astype(np.float32),
               out=torch.zeros(3, 40, device=DEV), accumulate=True, nsplit=nsplit)
    assert torch.isnan(got).all()


def test_adjoint_on_the_device():
    """|<A v, h> - <v, A^T h>| (float64 inner products of the fp32 outputs) within what the two bounds allow."""
    from nlosgr.backproject import backproject, fp32_window
    c = _problem((9, 5, 13), 257, 40, 0.3)
    g = np.random.default_rng(11)
    h = g.standard_normal((c["nwall"], c["nr"])).astype(np.float32)
    r0, inv_dr = fp32_window(c["r0"], c["dr"])
    grid = _grid(c["tabs"])
    for power in (0, 2, 4):
        _, Bf = _oracle(c, power)
        _, Bb = BO.backproject64(h, c["walls"], *c["tabs"], r0, inv_dr, power, d=c["d"])
        Av = _gpu(c, power, grid=grid).cpu().numpy().astype(np.float64)
        Ath = backproject(_dev(h), _dev(c["walls"]), grid, c["r0"], c["dr"], power=power).cpu().numpy().astype(np.float64)
        lhs, rhs = float((Av * h).sum()), float((c["vol"].astype(np.float64) * Ath).sum())
        tol = float((Bf * np.abs(h)).sum() + (np.abs(c["vol"]) * Bb).sum())
        print(f"adjoint power {power}: <Av,h> {lhs:.9g} <v,Ath> {rhs:.9g} difference / allowed {abs(lhs - rhs) / tol:.4f}")
        assert abs(lhs - rhs) <= tol


def test_against_the_renderer():
    """One Gaussian (std 0.03, albedo 1) at the centre of voxel (30, 20, 18) of the 49^3 grid, cuda preset, no
    occlusion, dense, a 2 x 2 wall, 32 x 32 rays per wall point, 80 bins: voxelize -> voxel_transient against
    render_forward.  The same comparison between the float64 oracles (tests/volume_oracle.py render against
    forward64 on tests/voxel_oracle.py's volume) gives the reference rel-L2; the factor 1.5 covers the renderer's
    own 32 x 32 angular quadrature, which the voxel path does not share."""
    import nlosgr
    import volume_oracle as VOL
    import voxel_oracle as VO
    from nlosgr.backproject import fp32_window
    from nlosgr.forward_project import voxel_transient
    from nlosgr.geometry import build_geometry, relay_wall_grid, volume_box_point
    from nlosgr.render import RenderConfig, render_forward
    from nlosgr.voxelize import VoxelGrid, voxelize
    S = BO.SCENE
    n, vi = 49, (30, 20, 18)
    dev = torch.device(DEV)
    grid = VoxelGrid(S["position"], S["size"], n)
    tabs = [t.numpy() for t in grid.tables]
    mu = torch.tensor([[tabs[0][vi[0]], tabs[1][vi[1]], tabs[2][vi[2]]]], dtype=torch.float32, device=dev)
    model = nlosgr.GaussianParams(mu, torch.full((1, 3), math.log(0.03), device=dev),
                                  torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev), torch.tensor([[4.0]], device=dev),
                                  torch.full((1, 1, 1), 0.5 / 0.28209479177387814, device=dev),
                                  torch.zeros(1, 0, 1, device=dev), 0, 0)
    walls = relay_wall_grid(2, 2, device=dev)
    c, dT, start, end = 1.0, 0.01, 20, 100
    geo = build_geometry(walls, volume_box_point(S["position"], S["size"], dev), 32, start, end, c, dT,
                         S["position"][1], "cuda")
    cfg = RenderConfig(preset="cuda", mode="noocl", sh_degree=0, c_deltaT=c * dT)
    hist, _ = render_forward(model._mu, model._scaling, model._rotation, model._opacity, nlosgr.features_flat(model),
                             geo, cfg)
    cam = torch.zeros(3, device=dev)
    _, alb = voxelize(model, grid, cam, preset="cuda", cutoff=0.0, sh_degree=0)
    got = voxel_transient(alb, grid, walls, geo.r, c * dT, S["position"][1])
    assert got.shape == hist.shape == (4, end - start)
    rel = ((got - hist).double().norm() / hist.double().norm()).item()
    # the float64 oracles on the same scene
    P = VO.params_of(model, 0, double=True)
    ref_hist = VOL.forward(P, geo, "cuda", "noocl", c * dT, 0.0).numpy()
    alb64 = VO.volumes(P, grid.coords(), cam.cpu(), "cuda", 1.0, None)[1].numpy()
    r = geo.r.double().cpu().numpy()
    nr = r.shape[0]
    r0, dr = float(r[0]), (float(r[-1]) - float(r[0])) / (nr - 1)
    rows64, _ = FO.forward64(alb64, walls.cpu().numpy(), *tabs, *fp32_window(r0, dr), nr, -4, want_bound=False)
    dv = np.prod([(float(t[-1]) - float(t[0])) / (len(t) - 1) for t in tabs])
    ref_vt = S["position"][1] ** 2 * (c * dT / dr) * dv * rows64
    rel64 = float(np.linalg.norm(ref_vt - ref_hist) / np.linalg.norm(ref_hist))
    print(f"voxel_transient against the renderer: rel-L2 {rel:.4f}; float64 oracles {rel64:.4f}")
    assert rel64 <= 0.1
    assert rel <= 1.5 * rel64
    assert (got.argmax(dim=1) - hist.argmax(dim=1)).abs().max().item() <= 1
    assert hist.max().item() > 0


def test_landweber_on_the_device():
    """The least-squares volume of the point-scatterer capture: the assertions of the float64 run
    (test_forward_project_cpu.py), and operator_norm against its eigenvalue."""
    from nlosgr.forward_project import landweber, operator_norm
    rows, walls, tabs, r0, inv_dr = BO.scatterer_scene()
    S = BO.SCENE
    grid = _grid(tabs)
    _, _, lam64 = FO.landweber64(rows, walls, tabs, r0, inv_dr, iterations=0)
    lam = operator_norm(_dev(walls), grid, S["r0"], S["dr"], S["nr"])
    print(f"operator_norm {lam:.3f} (float64 {lam64:.3f})")
    assert abs(lam - lam64) <= 1e-4 * lam64
    vol, obj = landweber(_dev(rows), _dev(walls), grid, S["r0"], S["dr"], iterations=30)
    assert obj.shape == (30,) and obj.is_cuda and vol.shape == (17, 17, 17) and (vol >= 0).all()
    o = obj.cpu().numpy()
    x = vol.cpu().numpy()
    top = np.sort(x.reshape(-1))
    print(f"landweber: objective {o[0]:.2f} -> {o[-1]:.2f}, runner-up / peak {top[-2] / top[-1]:.3f}")
    assert np.all(np.diff(o) < 0)
    assert o[-1] <= 0.6 * o[0]
    assert int(x.argmax()) == 3267
    assert top[-2] <= 0.25 * top[-1]


def test_command_line_writes_volume_and_mesh(tmp_path):
    """python -m nlosgr.forward_project (its main(), in process) on a written capture: the npz carries the key
    names of python -m nlosgr.backproject plus the objective, and the volume of landweber_capture; --mesh writes a
    readable PLY."""
    from nlosgr.data import make_data_kwargs, save_zaragoza
    from nlosgr.forward_project import landweber_capture, main
    from nlosgr.mesh import read_ply
    rows, walls, tabs, r0, inv_dr = BO.scatterer_scene()
    S = BO.SCENE
    data = np.zeros((100, 16, 16), dtype=np.float32)
    data[20:100] = rows.T.reshape(80, 16, 16)
    cap, out, ply = str(tmp_path / "cap.mat"), str(tmp_path / "lw.npz"), str(tmp_path / "lw.ply")
    save_zaragoza(cap, data, walls.T, S["position"], S["size"], 0.01, 1.0)
    main([cap, "--resolution", "17", "--start", "20", "--end", "100", "--iterations", "6", "--out", out, "--mesh", ply])
    z = np.load(out)
    assert sorted(z.files) == sorted(["density", "albedo", "front", "depth", "xs", "ys", "zs", "cam", "objective"])
    assert z["objective"].shape == (6,) and np.all(np.diff(z["objective"]) < 0)
    dk, *_ = make_data_kwargs(cap, DEV, shuffle=False)
    want = landweber_capture(dk, 17, 20, 100, iterations=6)
    assert np.array_equal(z["density"], want["volume"].cpu().numpy())
    assert np.array_equal(z["objective"], want["objective"].cpu().numpy()) and np.array_equal(z["albedo"], z["density"])
    assert np.array_equal(z["front"], z["density"].max(axis=1)) and np.array_equal(z["xs"], tabs[0])
    assert np.unravel_index(z["density"].argmax(), (17, 17, 17)) == S["voxel"]
    mesh = read_ply(ply)
    assert mesh.vertices.shape[0] > 0 and mesh.faces.shape[0] > 0


def test_error_cases():
    from nlosgr.forward_project import forward_project, landweber, voxel_transient
    grid = _grid(_tables((4, 4, 4)))
    vol, walls = torch.zeros(4, 4, 4, device=DEV), torch.zeros(3, 3, device=DEV)
    with pytest.raises(RuntimeError):
        forward_project(vol.cpu(), walls, grid, 0.0, 0.01, 8)
    with pytest.raises(RuntimeError):
        forward_project(vol, walls.cpu(), grid, 0.0, 0.01, 8)
    with pytest.raises(RuntimeError):
        forward_project(vol.double(), walls, grid, 0.0, 0.01, 8)
    with pytest.raises(RuntimeError):
        forward_project(vol, walls, grid, 0.0, 0.01, 8, out=torch.zeros(3, 8))
    with pytest.raises(ValueError):
        forward_project(vol, walls, grid, 0.0, 0.01, 8, out=torch.zeros(3, 9, device=DEV))
    with pytest.raises(ValueError):
        forward_project(vol[:3], walls, grid, 0.0, 0.01, 8)
    with pytest.raises(ValueError):
        forward_project(vol, walls[:, :2], grid, 0.0, 0.01, 8)
    with pytest.raises(ValueError):
        forward_project(vol, walls, grid, 0.0, 0.0, 8)
    with pytest.raises(ValueError):
        forward_project(vol, walls, grid, 0.0, 0.01, 0)
    with pytest.raises(ValueError):
        forward_project(vol, walls, grid, 0.0, 0.01, 8, accumulate=True)
    with pytest.raises(TypeError):
        forward_project(vol, walls, (4, 4, 4), 0.0, 0.01, 8)
    with pytest.raises(RuntimeError, match="power"):
        forward_project(vol, walls, grid, 0.0, 0.01, 8, power=5)
    with pytest.raises(RuntimeError, match="r0 \\* inv_dr"):
        forward_project(vol, walls, grid, 0.01, 0.01, 8, power=-4)
    with pytest.raises(RuntimeError, match="NLOSGR_IRF_MAX_NR"):
        forward_project(vol, walls, grid, 0.0, 0.01, 8193)
    with pytest.raises(RuntimeError, match="nsplit"):
        forward_project(vol, walls, grid, 0.0, 0.01, 8, nsplit=-1)
    with pytest.raises(ValueError):
        landweber(torch.zeros(3, 8, device=DEV), walls, grid, 0.0, 0.01, power=-1)
    with pytest.raises(ValueError):
        landweber(torch.zeros(2, 8, device=DEV), walls, grid, 0.0, 0.01)
    with pytest.raises(ValueError):
        voxel_transient(vol, grid, walls, torch.tensor([0.2]), 0.01, 0.5)
