"""GPU checks of the back-projection (include/nlosgr.h ABI 13, csrc/nlosgr_backproject.hip) against the float64
oracle of tests/backproject_oracle.py: |gpu - oracle| <= B per voxel, with B the oracle's derived bound and no
further factor.  `-s` prints the worst measured e/B per case.

Shapes are the smallest at which the kernel can go wrong: grid extents off and on the 8^3 brick, an odd z extent
for the two-voxels-per-lane pairing, wall counts around the 256-point LDS tile, a short and a long row, r0 = 0
and > 0, every power, rows with both signs.  The volume reaches in front of the window and behind it, so voxels
before the first bin, on either end ramp and past the last bin all occur, and voxel (0, 0, 0) sits on wall point 0
(d = 0)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import backproject_oracle as BO
import irf_oracle as IO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRIDS = [(1, 1, 1), (9, 5, 13), (17, 8, 3), (16, 16, 16)]
WALLS = [1, 255, 256, 257, 600]
NRS = [40, 1024]
R0S = [0.0, 0.3]
FAR = 0.9           # radius of the window's end: the farthest voxel is 1.28 from the farthest wall point
CASES = [(g, nw, nr, r0) for g in GRIDS for nw in WALLS for nr in NRS for r0 in R0S]


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
    return VoxelGrid(tables=[torch.from_numpy(t) for t in tabs])


def _problem(shape, nwall, nr, r0, seed=0):
    g = np.random.default_rng(seed + 1000 * nwall + nr + sum(shape))
    tabs = _tables(shape)
    walls = _walls(nwall, tabs, g)
    rows = g.standard_normal((nwall, nr)).astype(np.float32)
    dr = (FAR - r0) / nr
    return dict(shape=shape, nwall=nwall, nr=nr, r0=r0, dr=dr, tabs=tabs, walls=walls, rows=rows,
                d=BO.distances64(walls, *tabs))


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"g{'x'.join(map(str, p[0]))}-w{p[1]}-nr{p[2]}-r{p[3]}")
def case(request):
    return _problem(*request.param)


def _gpu(c, power=0, rows=None, walls=None, grid=None, **kw):
    from nlosgr.backproject import backproject
    rows = c["rows"] if rows is None else rows
    walls = c["walls"] if walls is None else walls
    return backproject(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV),
                       torch.from_numpy(np.ascontiguousarray(walls)).to(DEV), grid or _grid(c["tabs"]), c["r0"], c["dr"],
                       power=power, **kw)


def _oracle(c, power, rows=None, d=None, walls=None, **kw):
    from nlosgr.backproject import fp32_window
    r0, inv_dr = fp32_window(c["r0"], c["dr"])
    walls = c["walls"] if walls is None else walls
    return BO.backproject64(c["rows"] if rows is None else rows, walls, *c["tabs"], r0, inv_dr, power,
                            d=c["d"] if d is None and walls is c["walls"] else d, **kw)


def _share(err, B):
    m = B > 0
    return float((err[m] / B[m]).max()) if m.any() else 0.0


def test_parity_within_the_bound(case):
    worst = []
    for power in range(5):
        ref, B = _oracle(case, power)
        got = _gpu(case, power).cpu().numpy().astype(np.float64)
        assert got.shape == case["shape"] and np.isfinite(got).all()
        err = np.abs(got - ref)
        worst.append(_share(err, B))
        assert np.all(err <= B), (power, worst[-1])
    print(f"grid {case['shape']} walls {case['nwall']} nr {case['nr']} r0 {case['r0']}: worst e/B per power "
          + " ".join(f"{w:.4f}" for w in worst))


@pytest.mark.parametrize("nr", [1, 2, 3])
def test_shortest_rows(nr):
    """Rows of one, two and three bins: a one-bin row is read bin by bin, longer rows through the 8-byte read of
    two neighbouring bins, whose clamp range [0, nr - 2] is a single position at nr = 2."""
    c = _problem((9, 5, 13), 257, nr, 0.3)
    for power in (0, 3):
        ref, B = _oracle(c, power)
        got = _gpu(c, power).cpu().numpy().astype(np.float64)
        err = np.abs(got - ref)
        print(f"nr {nr} power {power}: worst e/B {_share(err, B):.4f}")
        assert np.isfinite(got).all() and ref.any() and np.all(err <= B)


def test_cases_reach_every_part_of_the_window():
    """The placement the parity cases rely on, checked once on the oracle's bin coordinate."""
    from nlosgr.backproject import fp32_window
    c = _problem((9, 5, 13), 600, 40, 0.3)
    u = BO.bin_coordinate(c["d"], *fp32_window(c["r0"], c["dr"]))
    nr = c["nr"]
    assert (u <= -1).any() and ((u > -1) & (u < 0)).any() and ((u >= 0) & (u <= nr - 1)).any()
    assert ((u > nr - 1) & (u < nr)).any() and (u >= nr).any()
    assert c["d"][0, 0] == 0.0
    one = _problem((9, 5, 13), 1, 40, 0.3)                       # a single wall point: whole voxels are dark
    u1 = BO.bin_coordinate(one["d"], *fp32_window(one["r0"], one["dr"]))[:, 0]
    got = _gpu(one).cpu().numpy().reshape(-1)
    assert (u1 <= -1).any() and not got[u1 <= -1].any() and (u1 >= nr).any() and not got[u1 >= nr].any()
    assert got[(u1 > 0) & (u1 < nr - 1)].all()


def test_repeatable_and_independent_of_bricks():
    """Two runs are bitwise equal, and sub-grids at offsets that are no brick multiples (odd z offsets: every
    voxel changes its lane, its pair partner and its brick) reproduce the full run's voxels bitwise."""
    c = _problem((19, 10, 21), 300, 40, 0.3)
    grid = _grid(c["tabs"])
    for power in (0, 3):
        full = _gpu(c, power, grid=grid)
        assert torch.equal(full, _gpu(c, power, grid=grid))
        for ix, iy, iz in (((3, 17), (1, 8), (5, 20)), ((9, 19), (0, 10), (11, 21)), ((7, 8), (2, 3), (20, 21))):
            sub = _gpu(c, power, grid=grid.slice(ix, iy, iz))
            assert torch.equal(sub, full[slice(*ix), slice(*iy), slice(*iz)]), (power, ix, iy, iz)


def test_accumulate_and_overwrite():
    c = _problem((9, 5, 13), 600, 40, 0.3)
    grid = _grid(c["tabs"])
    for power in (0, 2):
        ref, B = _oracle(c, power)
        one = _gpu(c, power, grid=grid)
        acc = _gpu(c, power, rows=c["rows"][:300], walls=c["walls"][:300], grid=grid)
        same = _gpu(c, power, rows=c["rows"][300:], walls=c["walls"][300:], grid=grid, out=acc, accumulate=True)
        assert same is acc
        a, o = acc.cpu().numpy(), one.cpu().numpy()
        ulp = np.spacing(np.abs(o)).astype(np.float64)
        diff = np.abs(a.astype(np.float64) - o.astype(np.float64))
        print(f"accumulate power {power}: worst |halves - one| / (B + ulp) {float((diff / (B + ulp)).max()):.4f}")
        assert np.all(diff <= B + ulp)
        assert np.all(np.abs(a.astype(np.float64) - ref) <= B + ulp)
        filled = torch.full(c["shape"], float("nan"), device=DEV)
        assert torch.equal(_gpu(c, power, grid=grid, out=filled), one) and torch.equal(filled, one)
    # no wall points: zero-fill, or untouched with accumulate
    empty = dict(c, rows=c["rows"][:0], walls=c["walls"][:0])
    z = _gpu(empty, grid=grid, out=torch.full(c["shape"], 7.0, device=DEV))
    assert not z.any()
    keep = _gpu(empty, grid=grid, out=torch.full(c["shape"], 7.0, device=DEV), accumulate=True)
    assert (keep == 7.0).all()


def test_nan_bin_reaches_the_voxels_that_sample_it():
    """A NaN in bin b of wall point i: voxels whose u_i lies inside (b-1, b+1) sample it and become NaN, voxels
    outside [b-1, b+1] come out as if the bin were 0.  Voxels within 1e-3 bins of either limit are left out: there
    the fp32 u (error ~5e-5 bins here) may fall on either side."""
    from nlosgr.backproject import fp32_window
    c = _problem((9, 5, 13), 257, 40, 0.3)
    i, b, m = 130, 17, 1e-3
    rows = c["rows"].copy()
    rows[i, b] = np.nan
    clean = c["rows"].copy()
    clean[i, b] = 0.0
    u = BO.bin_coordinate(c["d"][:, i], *fp32_window(c["r0"], c["dr"])).reshape(c["shape"])
    hit, miss = np.abs(u - b) < 1 - m, np.abs(u - b) > 1 + m
    assert hit.sum() >= 10 and miss.sum() >= 10 and (hit | miss).mean() > 0.99
    for power in (0, 1):
        got = _gpu(c, power, rows=rows).cpu().numpy()
        assert np.isnan(got[hit]).all() and np.isfinite(got[miss]).all()
        ref, B = _oracle(c, power, rows=clean)
        assert np.all(np.abs(got[miss].astype(np.float64) - ref[miss]) <= B[miss])
    inf = c["rows"].copy()
    inf[i, b] = np.inf
    got = _gpu(c, 0, rows=inf).cpu().numpy()
    assert not np.isfinite(got[hit]).any() and np.isfinite(got[miss]).all()


def test_point_scatterer_peaks_at_its_voxel():
    from nlosgr.backproject import backproject
    rows, walls, tabs, r0, inv_dr = BO.scatterer_scene()
    ref, B = BO.backproject64(rows, walls, *tabs, r0, inv_dr, 0)
    got = backproject(torch.from_numpy(rows).to(DEV), torch.from_numpy(walls).to(DEV), _grid(tabs), BO.SCENE["r0"],
                      BO.SCENE["dr"]).cpu().numpy()
    assert np.unravel_index(ref.argmax(), ref.shape) == BO.SCENE["voxel"]
    assert np.unravel_index(got.argmax(), got.shape) == BO.SCENE["voxel"]
    assert np.all(np.abs(got.astype(np.float64) - ref) <= B)


def _capture_kwargs(rows, walls, start, total_bins, hw, c=1.0, deltaT=0.01, dev=DEV):
    """data_kwargs of a capture whose bins [start, start + nr) hold rows [H*W, nr] (zero elsewhere)."""
    H, W = hw
    nr = rows.shape[1]
    data = torch.zeros(total_bins, H, W)
    data[start:start + nr] = torch.as_tensor(rows).t().reshape(nr, H, W)
    S = BO.SCENE
    vp = torch.tensor(S["position"], dtype=torch.float32, device=dev)
    pmin = torch.cat([vp - S["size"] / 2, torch.tensor([0.0, -np.pi], device=dev)])
    pmax = torch.cat([vp + S["size"] / 2, torch.tensor([np.pi, 0.0], device=dev)])
    return {"nlos_data": data.to(dev), "camera_grid_positions": torch.as_tensor(walls).t().contiguous().to(dev),
            "volume_position": vp, "volume_size": S["size"], "deltaT": deltaT, "c": c, "pmin": pmin, "pmax": pmax}


def test_against_the_renderer():
    """One compact Gaussian (std 0.02, two thirds of a voxel) at the centre of voxel (11, 5, 3) of the 17^3 grid,
    rendered by the volume forward (dense, cuda preset, no occlusion; 16 x 16 wall, 32 x 32 rays per wall point,
    bins 20..100 of c deltaT = 0.01), then back-projected unfiltered: the GPU's argmax is the oracle's on the same
    rows, and that lies within one voxel (Chebyshev) of the mean (on the float64 render of the same scene it is
    the mean's own voxel)."""
    import nlosgr
    from nlosgr.backproject import backproject_capture, fp32_window
    from nlosgr.geometry import build_geometry, relay_wall_grid, volume_box_point
    from nlosgr.render import RenderConfig, render
    S = BO.SCENE
    tabs = BO.linspace_tables(S["position"], S["size"], S["res"])
    vi = S["voxel"]
    dev = torch.device(DEV)
    mu = torch.tensor([[tabs[0][vi[0]], tabs[1][vi[1]], tabs[2][vi[2]]]], dtype=torch.float32, device=dev)
    model = nlosgr.GaussianParams(mu, torch.full((1, 3), math.log(0.02), device=dev),
                                  torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev), torch.tensor([[4.0]], device=dev),
                                  torch.full((1, 1, 1), 0.5 / 0.28209479177387814, device=dev),
                                  torch.zeros(1, 0, 1, device=dev), 0, 0)
    walls = relay_wall_grid(16, 16, device=dev)
    c, dT, start, end = 1.0, 0.01, 20, 100
    geo = build_geometry(walls, volume_box_point(S["position"], S["size"], dev), 32, start, end, c, dT,
                         S["position"][1], "cuda")
    cfg = RenderConfig(preset="cuda", mode="noocl", sh_degree=0, c_deltaT=c * dT)
    with torch.no_grad():
        hist, _ = render(model._mu, model._scaling, model._rotation, model._opacity, nlosgr.features_flat(model), geo, cfg)
    assert hist.shape == (256, end - start) and hist.max().item() > 0
    dk = _capture_kwargs(hist.cpu(), walls.cpu(), start, end + 4, (16, 16), c, dT)
    out = backproject_capture(dk, S["res"], start, end, filter="none")
    got = out["volume"].cpu().numpy()
    ref, B = BO.backproject64(hist.cpu().numpy(), walls.cpu().numpy(), *tabs, *fp32_window(start * c * dT, c * dT), 0)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= B)
    peak = np.unravel_index(ref.argmax(), ref.shape)
    assert np.unravel_index(got.argmax(), got.shape) == peak
    assert max(abs(int(a) - b) for a, b in zip(peak, vi)) <= 1, peak
    assert out["grid"].shape == (17, 17, 17) and out["front"].shape == (17, 17) and out["depth"].shape == (17, 17)
    assert torch.equal(out["front"], out["volume"].max(dim=1).values)
    assert out["depth"][peak[0], peak[2]].item() == float(tabs[1][peak[1]])


def test_filtered_back_projection():
    """backproject(irf_apply(rows, time_filter("log"))) against the oracle fed the float64-filtered rows.  The
    bound is B of those rows plus the IRF test's own tolerance, (L + 2) 2^-24 (|w| * |h|) per filtered bin
    (tests/irf_oracle.py apply_bound), carried through the back-projection (its weights are >= 0, so the
    back-projection of the per-bin tolerance bounds the effect of the filter's fp32 error)."""
    from nlosgr.backproject import time_filter
    from nlosgr.irf import irf_apply
    c = _problem((9, 5, 13), 257, 120, 0.3)
    filt = time_filter("log", sigma_bins=2.0)
    w = filt.taps.numpy()
    y64 = IO.apply64(c["rows"], w, filt.center, 0.0)
    ybound, _ = IO.apply_bound(c["rows"], w, filt.center, 0.0)
    y = irf_apply(torch.from_numpy(c["rows"]).to(DEV), filt)
    assert np.all(np.abs(y.cpu().numpy().astype(np.float64) - y64) <= ybound)
    for power in (0, 2):
        ref, B = _oracle(c, power, rows=y64)
        tol, _ = _oracle(c, power, rows=ybound, want_bound=False)
        got = _gpu(c, power, rows=y.cpu().numpy()).cpu().numpy().astype(np.float64)
        err = np.abs(got - ref)
        print(f"filtered power {power}: worst e/(B + filter) {_share(err, B + tol):.4f}")
        assert np.all(err <= B + tol)
    # the Laplacian filter through the same path
    lap = time_filter("laplacian")
    y64 = IO.apply64(c["rows"], lap.taps.numpy(), 1, 0.0)
    ybound, _ = IO.apply_bound(c["rows"], lap.taps.numpy(), 1, 0.0)
    ref, B = _oracle(c, 0, rows=y64)
    tol, _ = _oracle(c, 0, rows=ybound, want_bound=False)
    got = _gpu(c, 0, rows=irf_apply(torch.from_numpy(c["rows"]).to(DEV), lap).cpu().numpy()).cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - ref) <= B + tol)


def _inside_box(dk, grid, margin):
    pmin, pmax = dk["pmin"][:3].cpu().numpy(), dk["pmax"][:3].cpu().numpy()
    lo, hi = pmin + np.abs(pmin * margin), pmax - np.abs(pmax * margin)
    m = [(t.numpy() >= lo[a]) & (t.numpy() <= hi[a]) for a, t in enumerate(grid.tables)]
    return m[0][:, None, None] & m[1][None, :, None] & m[2][None, None, :]


def test_initialiser_on_the_golden_capture():
    import os
    from conftest import GOLDEN
    from nlosgr.backproject import backproject_capture
    from nlosgr.init import sample_from_backprojection
    z = np.load(os.path.join(GOLDEN, "carving.npz"), allow_pickle=False)
    vp = torch.from_numpy(z["volume_position"]).float().to(DEV)
    vs = float(z["volume_size"])
    dk = {"nlos_data": torch.from_numpy(z["nlos_data"]).to(DEV), "camera_grid_positions": torch.from_numpy(z["walls"]).to(DEV),
          "volume_position": vp, "volume_size": vs, "deltaT": float(z["deltaT"]), "c": float(z["c"]),
          "pmin": torch.cat([vp - vs / 2, torch.tensor([0.0, -np.pi], device=DEV)]),
          "pmax": torch.cat([vp + vs / 2, torch.tensor([np.pi, 0.0], device=DEV)])}
    n = int(z["carving_volume_size"])
    args = SimpleNamespace(init_gaussian_num=500, carving_volume_size=n)
    np.random.seed(0)
    torch.manual_seed(0)
    pts, rho = sample_from_backprojection(args, dk, margin=0.1, rho_scale=0.2)
    assert pts.shape == (500, 3) and pts.is_cuda and rho.shape == (500, 1) and (0 <= rho).all() and (rho <= 0.2).all()
    out = backproject_capture(dk, n, 0, z["nlos_data"].shape[0], filter="log")
    ok = torch.from_numpy(_inside_box(dk, out["grid"], 0.1)).to(DEV) & (out["volume"] > 0)
    assert 0 < ok.sum().item() < ok.numel()
    allowed = out["grid"].coords().to(DEV)[ok]                           # [K, 3]
    half = vs / (n - 1) / 2
    dist = (pts[:, None, :] - allowed[None]).abs().amax(-1).amin(1)     # Chebyshev distance to an allowed voxel
    assert (dist <= half + 1e-5).all()


@pytest.mark.parametrize("gamma", [1.0, 2.0])
def test_initialiser_finds_the_point_scatterer(gamma):
    """500 draws on the point-scatterer capture (default filter "log").  The share of the oracle volume's own
    probability within two voxels (Chebyshev) of the scatterer is 0.431 at gamma = 1 and 0.847 at gamma = 2
    (a uniform draw inside the margin box gives 0.04): below the 0.9 a sharper volume would allow, so the test
    holds the draws to that share minus the binomial 4 sigma, 0.342 and 0.783."""
    from nlosgr.backproject import time_filter
    from nlosgr.init import sample_from_backprojection
    rows, walls, tabs, r0, inv_dr = BO.scatterer_scene()
    S = BO.SCENE
    start, nr, n = 20, S["nr"], 500
    dk = _capture_kwargs(rows, walls, start, start + nr, S["wall"])
    grid = _grid(tabs)
    filt = time_filter("log", sigma_bins=2.0)
    vol64, _ = BO.backproject64(IO.apply64(rows, filt.taps.numpy(), filt.center, 0.0), walls, *tabs, r0, inv_dr, 0,
                                want_bound=False)
    w = np.where(_inside_box(dk, grid, 0.1), np.maximum(vol64, 0.0), 0.0) ** gamma
    idx = np.stack(np.meshgrid(*(np.arange(S["res"]),) * 3, indexing="ij"), axis=-1)
    near = np.abs(idx - np.array(S["voxel"])).max(axis=-1) <= 2
    p = float((w * near).sum() / w.sum())
    want = min(0.9, p - 4.0 * math.sqrt(p * (1.0 - p) / n))
    args = SimpleNamespace(init_gaussian_num=n, carving_volume_size=S["res"], start=start, end=start + nr)
    np.random.seed(1)
    torch.manual_seed(1)
    pts, rho = sample_from_backprojection(args, dk, gamma=gamma)
    spacing = S["size"] / (S["res"] - 1)
    centre = torch.tensor([tabs[a][S["voxel"][a]] for a in range(3)], device=DEV)
    share = ((pts - centre[None]).abs().amax(-1) <= 2.5 * spacing + 1e-6).float().mean().item()
    print(f"gamma {gamma}: oracle share {p:.3f}, required {want:.3f}, drawn {share:.3f}")
    assert pts.shape == (n, 3) and rho.shape == (n, 1) and (rho <= 0.1).all()
    assert share >= want


def test_initialiser_refuses_a_dark_capture():
    from nlosgr.init import sample_from_backprojection
    rows, walls, tabs, r0, inv_dr = BO.scatterer_scene()
    dk = _capture_kwargs(np.zeros_like(rows), walls, 20, 100, BO.SCENE["wall"])
    args = SimpleNamespace(init_gaussian_num=10, carving_volume_size=9, start=20, end=100)
    with pytest.raises(RuntimeError, match="back-projection is zero"):
        sample_from_backprojection(args, dk)


def test_error_cases():
    from nlosgr.backproject import backproject, backproject_capture
    grid = _grid(_tables((4, 4, 4)))
    rows, walls = torch.zeros(3, 8, device=DEV), torch.zeros(3, 3, device=DEV)
    with pytest.raises(RuntimeError):
        backproject(rows.cpu(), walls, grid, 0.0, 0.01)
    with pytest.raises(RuntimeError):
        backproject(rows, walls.cpu(), grid, 0.0, 0.01)
    with pytest.raises(RuntimeError):
        backproject(rows.double(), walls, grid, 0.0, 0.01)
    with pytest.raises(RuntimeError):
        backproject(rows, walls, grid, 0.0, 0.01, out=torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError):
        backproject(rows, walls, grid, 0.0, 0.01, out=torch.zeros(4, 4, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        backproject(rows, walls, grid, 0.0, 0.01, out=torch.zeros(4, 4, 5, device=DEV))
    with pytest.raises(ValueError):
        backproject(rows, walls[:2], grid, 0.0, 0.01)
    with pytest.raises(ValueError):
        backproject(rows, walls, grid, 0.0, 0.0)
    with pytest.raises(ValueError):
        backproject(rows, walls, grid, 0.0, 0.01, accumulate=True)
    with pytest.raises(TypeError):
        backproject(rows, walls, (4, 4, 4), 0.0, 0.01)
    with pytest.raises(RuntimeError, match="power"):
        backproject(rows, walls, grid, 0.0, 0.01, power=5)
    with pytest.raises(ValueError):
        backproject_capture({}, 8, 0, 10, filter="box")


def test_command_line_writes_volume_and_mesh(tmp_path):
    """python -m nlosgr.backproject (its main(), in process) on a written capture: the npz carries the key names
    of python -m nlosgr.voxelize and the volume of backproject_capture; --mesh writes a readable PLY."""
    from nlosgr.backproject import backproject_capture, main
    from nlosgr.data import make_data_kwargs, save_zaragoza
    from nlosgr.mesh import read_ply
    rows, walls, tabs, r0, inv_dr = BO.scatterer_scene()
    S = BO.SCENE
    data = np.zeros((100, 16, 16), dtype=np.float32)
    data[20:100] = rows.T.reshape(80, 16, 16)
    cap, out, ply = str(tmp_path / "cap.mat"), str(tmp_path / "bp.npz"), str(tmp_path / "bp.ply")
    save_zaragoza(cap, data, walls.T, S["position"], S["size"], 0.01, 1.0)
    main([cap, "--resolution", "17", "--start", "20", "--end", "100", "--filter", "laplacian", "--out", out, "--mesh",
          ply, "--level-frac", "0.5"])
    z = np.load(out)
    assert sorted(z.files) == sorted(["density", "albedo", "front", "depth", "xs", "ys", "zs", "cam"])
    dk, *_ = make_data_kwargs(cap, DEV, shuffle=False)
    want = backproject_capture(dk, 17, 20, 100, filter="laplacian")
    assert np.array_equal(z["density"], want["volume"].cpu().numpy()) and np.array_equal(z["albedo"], z["density"])
    assert np.array_equal(z["front"], z["density"].max(axis=1)) and z["depth"].shape == (17, 17)
    assert np.array_equal(z["xs"], tabs[0]) and np.array_equal(z["ys"], tabs[1])
    assert np.unravel_index(z["density"].argmax(), (17, 17, 17)) == S["voxel"]
    mesh = read_ply(ply)
    assert mesh.vertices.shape[0] > 0 and mesh.faces.shape[0] > 0
