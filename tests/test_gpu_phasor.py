"""GPU checks of the phasor-field reconstruction (include/nlosgr.h nlosgr_backproject_phasor, csrc/
nlosgr_backproject.hip, nlosgr/phasor.py).  The reference for the planes is the existing real kernels: plane c is
BITWISE backproject() of channel c alone, so no tolerance is new here; each plane is also held to the float64
oracles' derived bound B (no factor), and mag to 1 fp32 ulp of float32(sqrt(float64(re)^2 + float64(im)^2)).

Shapes are the smallest at which the kernel can go wrong: a 17 x 9 x 7 grid (partial bricks on every axis, an odd nz
leaves the z pair's second voxel outside the grid), 261 = 256 + 4 + 1 measurements (a second tile, one full group,
one remainder), 80 bins with a window the volume overshoots at both ends, and rows of one and two bins (the edge
cases of the 16-byte read)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import backproject_oracle as BO
import nonconfocal_oracle as NO
import phasor_oracle as PO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ["confocal", "per_meas", "one_laser"]
WAVELENGTH, CYCLES = 0.16, 4.0


def _problem(shape, nmeas, nr):
    """NO.problem with complex rows [nmeas, nr, 2] (seeded normal) beside it."""
    c = NO.problem(shape, nmeas, nr, 0.3)
    c["rows_c"] = np.random.default_rng(77 + nmeas + nr).standard_normal((nmeas, nr, 2)).astype(np.float32)
    return c


@pytest.fixture(scope="module")
def mid():
    return _problem((17, 9, 7), 261, 80)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _grid(tabs):
    from nlosgr.voxelize import VoxelGrid
    return VoxelGrid(tables=[torch.from_numpy(np.ascontiguousarray(t)) for t in tabs])


def _lasers(c, mode, sl=slice(None)):
    """The lasers of a mode as numpy: None, [nmeas, 3] (rows sl) or [1, 3]."""
    return None if mode == "confocal" else (c["lasers"][sl] if mode == "per_meas" else c["lasers"][:1])


def _ph(c, mode, power=0, rows_c=None, sl=slice(None), grid=None, lasers="mode", **kw):
    from nlosgr.phasor import phasor_backproject
    rows_c = c["rows_c"] if rows_c is None else rows_c
    lasers = _lasers(c, mode, sl) if isinstance(lasers, str) else lasers
    return phasor_backproject(_dev(rows_c[sl]), _dev(c["sensors"][sl]), grid or _grid(c["tabs"]), c["r0"], c["dr"],
                              power=power, lasers=None if lasers is None else _dev(lasers), **kw)


def _bp(c, mode, ch, power=0, rows_c=None, sl=slice(None), grid=None, **kw):
    """The real kernels on one channel of the complex rows."""
    from nlosgr.backproject import backproject
    rows_c = c["rows_c"] if rows_c is None else rows_c
    lasers = _lasers(c, mode, sl)
    return backproject(_dev(rows_c[sl][..., ch]), _dev(c["sensors"][sl]), grid or _grid(c["tabs"]), c["r0"], c["dr"],
                       power=power, lasers=None if lasers is None else _dev(lasers), **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ulps(got, want):
    """Largest distance in fp32 ulps between two non-negative finite fp32 arrays, and the count of differing ones."""
    g, w = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert np.isfinite(g).all() and np.isfinite(w).all() and (g >= 0).all() and (w >= 0).all()
    d = np.abs(g.view(np.int32).astype(np.int64) - w.view(np.int32).astype(np.int64))
    return int(d.max()) if d.size else 0, int((d != 0).sum())


def _u64(c, mode):
    ds, dl = c["d"]
    r0, inv_dr = NO.window(c)
    if mode == "confocal":
        return BO.bin_coordinate(ds, r0, inv_dr)
    if mode == "one_laser":
        dl = np.broadcast_to(dl[:, :1], ds.shape)
    return NO.bin_coordinate(ds, dl, r0, inv_dr)


@pytest.mark.parametrize("mode", MODES)
def test_planes_are_bitwise_the_real_kernels(mid, mode):
    nr = mid["nr"]
    u = _u64(mid, mode)
    # both window edges and both e = +-1 selects are hit
    assert (u < -1).any() and (u > nr).any() and ((u > -1) & (u < 0)).any() and ((u > nr - 1) & (u < nr)).any()
    for power in range(5):
        planes, mag = _ph(mid, mode, power)
        assert planes.shape == (2, 17, 9, 7) and mag.shape == (17, 9, 7) and planes.is_contiguous()
        for ch in range(2):
            want = _bp(mid, mode, ch, power)
            assert want.any() and torch.isfinite(want).all()
            assert torch.equal(planes[ch], want), (mode, power, ch)


@pytest.mark.parametrize("nr", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_shortest_rows(mode, nr):
    c = _problem((9, 8, 7), 5, nr)
    for power in (0, 1, 4):
        planes, mag = _ph(c, mode, power)
        for ch in range(2):
            want = _bp(c, mode, ch, power)
            assert torch.equal(planes[ch], want), (mode, nr, power, ch)
        assert planes.any()
        assert _ulps(mag.cpu().numpy(), PO.magnitude32(planes[0].cpu().numpy(), planes[1].cpu().numpy()))[0] <= 1


@pytest.mark.parametrize("mode", MODES)
def test_nan_and_inf_bins_stay_in_their_channel(mid, mode):
    rows_c = mid["rows_c"].copy()
    rows_c[3, 17, 0] = np.nan
    rows_c[200, 40, 1] = np.inf
    for power in (0, 3):
        planes, mag = _ph(mid, mode, power, rows_c=rows_c)
        nan = torch.isnan(planes)
        assert nan[0].any() and not nan[0].all() and not torch.isfinite(planes[1]).all()
        for ch in range(2):
            assert _same_bits(planes[ch], _bp(mid, mode, ch, power, rows_c=rows_c)), (mode, power, ch)
        assert torch.equal(torch.isnan(mag), nan[0] | nan[1])
        # the NaN bin of the re channel reaches the im plane nowhere: im's NaNs are its own inf bin's (0 * inf)
        clean = rows_c.copy()
        clean[3, 17, 0] = 0.0
        assert _same_bits(planes[1], _ph(mid, mode, power, rows_c=clean)[0][1])


@pytest.mark.parametrize("mode", MODES)
def test_magnitude(mid, mode):
    worst, differing = 0, 0
    for power in (0, 2):
        planes, mag = _ph(mid, mode, power)
        want = PO.magnitude32(planes[0].cpu().numpy(), planes[1].cpu().numpy())
        u, n = _ulps(mag.cpu().numpy(), want)
        worst, differing = max(worst, u), differing + n
        only, none = _ph(mid, mode, power, magnitude=False)
        assert none is None and torch.equal(only, planes)
    print(f"{mode}: mag against float32(sqrt(float64(re)^2 + float64(im)^2)): worst {worst} ulp, {differing} voxels differ")
    assert worst <= 1


@pytest.mark.parametrize("mode", MODES)
def test_accumulate(mid, mode):
    a, b = slice(0, 256), slice(256, None)
    for power in (0, 3):
        planes, mag0 = _ph(mid, mode, power, sl=a)
        got, mag = _ph(mid, mode, power, sl=b, planes=planes, accumulate=True)
        assert got is planes
        for ch in range(2):
            want = _bp(mid, mode, ch, power, sl=a)
            _bp(mid, mode, ch, power, sl=b, out=want, accumulate=True)
            assert torch.equal(planes[ch], want), (mode, power, ch)
        assert not torch.equal(mag, mag0)
        assert _ulps(mag.cpu().numpy(), PO.magnitude32(planes[0].cpu().numpy(), planes[1].cpu().numpy()))[0] <= 1
    with pytest.raises(ValueError, match="accumulate"):
        _ph(mid, mode, accumulate=True)


@pytest.mark.parametrize("mode", ["confocal", "one_laser"])
def test_no_measurements(mid, mode):
    empty = slice(0, 0)
    planes = torch.full((2, 17, 9, 7), 7.0, device=DEV)
    got, mag = _ph(mid, mode, sl=empty, planes=planes)
    assert got is planes and not planes.any() and mag.shape == (17, 9, 7) and not mag.any()
    kept, _ = _ph(mid, mode, 2)
    before = kept.clone()
    _, mag = _ph(mid, mode, 2, sl=empty, planes=kept, accumulate=True)
    assert _same_bits(kept, before)
    assert _ulps(mag.cpu().numpy(), PO.magnitude32(before[0].cpu().numpy(), before[1].cpu().numpy()))[0] <= 1
    assert _ph(mid, mode, sl=empty, magnitude=False)[1] is None


@pytest.mark.parametrize("mode", MODES)
def test_planes_within_the_float64_bound(mid, mode):
    r0, inv_dr = NO.window(mid)
    worst = []
    for power in range(5):
        ref, B, _ = PO.backproject64(mid["rows_c"], mid["sensors"], *mid["tabs"], r0, inv_dr, power,
                                     lasers=_lasers(mid, mode))
        planes, _ = _ph(mid, mode, power)
        err = np.abs(planes.cpu().numpy().astype(np.float64) - ref)
        m = B > 0
        worst.append(float((err[m] / B[m]).max()))
        assert np.all(err <= B), (mode, power, worst[-1])
    print(f"{mode}: worst e/B of either plane, powers 0..4: " + " ".join(f"{w:.4f}" for w in worst))


def test_phasor_rows_are_the_two_filtered_channels(mid):
    from nlosgr.irf import irf_apply
    from nlosgr.phasor import phasor_kernel, phasor_rows
    rows = _dev(mid["rows"])
    kc, ks = phasor_kernel(0.09, mid["dr"], 3.0)
    assert len(kc) == 19
    rc = phasor_rows(rows, (kc, ks))
    assert rc.shape == (261, 80, 2) and rc.is_contiguous() and rc.dtype == torch.float32
    assert torch.equal(rc[..., 0], irf_apply(rows, kc)) and torch.equal(rc[..., 1], irf_apply(rows, ks))
    assert rc[..., 1].any()


def _scatterer_argmax(rows, walls, lasers, tabs, r0):
    from nlosgr.phasor import phasor_backproject, phasor_kernel, phasor_rows
    dr = BO.SCENE["dr"]
    rc = phasor_rows(_dev(rows), phasor_kernel(WAVELENGTH, dr, CYCLES))
    planes, mag = phasor_backproject(rc, _dev(walls), _grid(tabs), r0, dr, lasers=None if lasers is None else _dev(lasers))
    return tuple(int(v) for v in np.unravel_index(int(mag.argmax()), tuple(mag.shape))), planes, mag


def test_point_scatterer_peaks_at_its_voxel():
    """End to end on the GPU: filter + gather + magnitude.  The float64 oracle's peak stands 1.153 x above the
    second-largest voxel (test_phasor_cpu.py), far more than fp32 moves any voxel."""
    rows, walls, tabs, r0, inv_dr = BO.scatterer_scene()
    at, planes, mag = _scatterer_argmax(rows, walls, None, tabs, BO.SCENE["r0"])
    assert at == BO.SCENE["voxel"] and torch.isfinite(mag).all()
    rows, sensors, lasers, tabs, r0, inv_dr = PO.nc_scatterer_scene()
    at, _, _ = _scatterer_argmax(rows, sensors, lasers, tabs, BO.SCENE["r0"])
    assert at == BO.SCENE["voxel"]


@pytest.mark.parametrize("mode", MODES)
def test_repeatable_and_independent_of_bricks(mid, mode):
    planes, mag = _ph(mid, mode, 3)
    again, mag2 = _ph(mid, mode, 3)
    assert torch.equal(planes, again) and torch.equal(mag, mag2)
    sub = _grid(mid["tabs"]).slice((3, 14), (1, 8), (2, 7))
    part, pmag = _ph(mid, mode, 3, grid=sub)
    assert part.shape == (2, 11, 7, 5)
    assert torch.equal(part, planes[:, 3:14, 1:8, 2:7]) and torch.equal(pmag, mag[3:14, 1:8, 2:7])
    if mode == "one_laser":
        many = np.ascontiguousarray(np.broadcast_to(mid["lasers"][:1], (mid["nmeas"], 3)))
        for power in (0, 3):
            a, am = _ph(mid, mode, power)
            b, bm = _ph(mid, mode, power, lasers=many)
            assert torch.equal(a, b) and torch.equal(am, bm)


def test_error_cases():
    from nlosgr.phasor import phasor_backproject
    grid = _grid(NO.tables((4, 4, 4)))
    rows_c, walls = torch.zeros(3, 8, 2, device=DEV), torch.zeros(3, 3, device=DEV)
    with pytest.raises(RuntimeError):
        phasor_backproject(rows_c.cpu(), walls, grid, 0.0, 0.01)
    with pytest.raises(RuntimeError):
        phasor_backproject(rows_c, walls.cpu(), grid, 0.0, 0.01)
    with pytest.raises(RuntimeError):
        phasor_backproject(rows_c.double(), walls, grid, 0.0, 0.01)
    with pytest.raises(RuntimeError):
        phasor_backproject(rows_c, walls, grid, 0.0, 0.01, lasers=walls.cpu())
    for bad in (torch.zeros(3, 8, device=DEV), torch.zeros(3, 8, 3, device=DEV), torch.zeros(2, 8, 2, device=DEV)):
        with pytest.raises(ValueError):
            phasor_backproject(bad, walls, grid, 0.0, 0.01)
    with pytest.raises(ValueError):
        phasor_backproject(rows_c, walls, grid, 0.0, 0.01, lasers=walls[:2])
    with pytest.raises(RuntimeError):
        phasor_backproject(rows_c, walls, grid, 0.0, 0.01, planes=torch.zeros(2, 4, 4, 4))
    with pytest.raises(RuntimeError):
        phasor_backproject(rows_c, walls, grid, 0.0, 0.01, planes=torch.zeros(2, 4, 4, 4, dtype=torch.float64, device=DEV))
    for shape in ((4, 4, 4), (2, 4, 4, 5), (1, 4, 4, 4)):
        with pytest.raises(ValueError):
            phasor_backproject(rows_c, walls, grid, 0.0, 0.01, planes=torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError):
        phasor_backproject(rows_c, walls, grid, 0.0, 0.0)
    with pytest.raises(ValueError):
        phasor_backproject(rows_c, walls, grid, 0.0, 0.01, accumulate=True)
    with pytest.raises(TypeError):
        phasor_backproject(rows_c, walls, (4, 4, 4), 0.0, 0.01)
    with pytest.raises(RuntimeError, match="power"):
        phasor_backproject(rows_c, walls, grid, 0.0, 0.01, power=5)


@pytest.mark.parametrize("kind", ["confocal", "lasers"])
def test_phasor_capture_and_the_initialiser(tmp_path, kind):
    """A tiny written capture (8 x 8 wall, SCENE's scatterer, bins [20, 100) of 100), confocal and with a laser
    per sensed point: the documented keys and shapes, the volume bitwise phasor_backproject's for the same rows,
    the command line's npz and PLY, and the initialiser's draws inside the shrunken box."""
    from nlosgr.backproject import capture_lasers
    from nlosgr.data import make_data_kwargs, save_zaragoza, volume_target
    from nlosgr.init import sample_from_backprojection
    from nlosgr.phasor import phasor_backproject, phasor_capture, phasor_kernel, phasor_rows
    from nlosgr.voxelize import VoxelGrid
    S = BO.SCENE
    walls = BO.relay_wall(8, 8)
    lasers = None if kind == "confocal" else (walls + np.asarray(PO.LASER_SHIFT, dtype=np.float32)[None]).astype(np.float32)
    tabs = BO.linspace_tables(S["position"], S["size"], 9)
    r0, inv_dr = BO.scene_window()
    point = (tabs[0][6], tabs[1][3], tabs[2][2])
    rows = (BO.scatterer_rows(walls, point, r0, inv_dr, S["nr"]) if lasers is None
            else NO.scatterer_rows(walls, lasers, point, r0, inv_dr, S["nr"])[0])
    data = np.zeros((100, 8, 8), dtype=np.float32)
    data[20:100] = rows.T.reshape(80, 8, 8)
    cap = str(tmp_path / "cap.mat")
    save_zaragoza(cap, data, walls.T, S["position"], S["size"], S["dr"], 1.0,
                  laser_grid_positions=None if lasers is None else lasers.T)
    dk, *_ = make_data_kwargs(cap, DEV, shuffle=False)
    assert (capture_lasers(dk) is None) == (lasers is None)
    out = phasor_capture(dk, 9, 20, 100, WAVELENGTH, cycles=CYCLES, power=1)
    assert sorted(out) == sorted(["volume", "real", "imag", "front", "depth", "grid"])
    assert out["volume"].shape == out["real"].shape == out["imag"].shape == (9, 9, 9)
    assert out["front"].shape == out["depth"].shape == (9, 9) and out["grid"].shape == (9, 9, 9)
    cdt = float(dk["c"]) * float(dk["deltaT"])
    rc = phasor_rows(volume_target(dk, 20, 80), phasor_kernel(WAVELENGTH, cdt, CYCLES))
    planes, mag = phasor_backproject(rc, dk["camera_grid_positions"].t().contiguous().float(),
                                     VoxelGrid(S["position"], S["size"], 9), 20 * cdt, cdt, power=1,
                                     lasers=capture_lasers(dk))
    assert torch.equal(out["volume"], mag) and torch.equal(out["real"], planes[0]) and torch.equal(out["imag"], planes[1])
    assert mag.any() and torch.equal(out["front"], mag.amax(dim=1))
    # python -m nlosgr.phasor (its main(), in process): the npz keys of python -m nlosgr.backproject plus the planes
    from nlosgr.mesh import read_ply
    from nlosgr.phasor import main
    npz, ply = str(tmp_path / "ph.npz"), str(tmp_path / "ph.ply")
    main([cap, "--resolution", "9", "--start", "20", "--end", "100", "--wavelength", str(WAVELENGTH), "--power", "1",
          "--out", npz, "--mesh", ply, "--level-frac", "0.5"])
    z = np.load(npz)
    assert sorted(z.files) == sorted(["density", "albedo", "front", "depth", "xs", "ys", "zs", "cam", "real", "imag"])
    assert np.array_equal(z["density"], mag.cpu().numpy()) and np.array_equal(z["albedo"], z["density"])
    assert np.array_equal(z["real"], planes[0].cpu().numpy()) and np.array_equal(z["imag"], planes[1].cpu().numpy())
    assert np.array_equal(z["xs"], tabs[0]) and read_ply(ply).vertices.shape[0] > 0
    args = SimpleNamespace(init_gaussian_num=200, carving_volume_size=9, start=20, end=100)
    np.random.seed(2)
    torch.manual_seed(2)
    pts, rho = sample_from_backprojection(args, dk, margin=0.1, wavelength=WAVELENGTH, cycles=CYCLES)
    assert pts.shape == (200, 3) and pts.is_cuda and rho.shape == (200, 1)
    pmin, pmax = dk["pmin"][:3], dk["pmax"][:3]
    lo, hi = pmin + (pmin * 0.1).abs(), pmax - (pmax * 0.1).abs()
    half = (pmax - pmin) / (9 - 1) / 2                                   # the jitter: half a grid spacing
    assert (pts >= lo - half - 1e-6).all() and (pts <= hi + half + 1e-6).all()
    spacing = S["size"] / 8
    centre = torch.tensor(point, device=DEV)
    near = ((pts - centre[None]).abs().amax(-1) <= 2.5 * spacing).float().mean().item()
    print(f"{kind}: share of the draws within two voxels of the scatterer {near:.3f}")
