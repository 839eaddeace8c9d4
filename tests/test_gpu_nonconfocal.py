"""GPU checks of the non-confocal back-projection and forward projection (include/nlosgr.h, csrc/
nlosgr_backproject.hip, csrc/nlosgr_forward_project.hip) against the float64 oracle of
tests/nonconfocal_oracle.py: |gpu - oracle| <= B per voxel
or bin, with B the oracle's derived bound and no further factor, and bitwise against the confocal entry points
where the laser spots are the sensed points.  `-s` prints the worst measured e/B per case.

Shapes are the smallest at which the kernels can go wrong: one voxel, grids off the 8^3 brick and off a lane's
run of 4 voxels, an odd z extent, 1, 3 and 257 measurements (257 crosses the 256-measurement tile and leaves a
workgroup of the forward projector with one measurement), rows of one and two bins (the edge cases of the 8-byte
read) and a short row, r0 = 0 and > 0, every power.  The volume reaches in front of the window and behind it, and
sensed point 0 sits on voxel (0, 0, 0)."""
import numpy as np
import pytest
import torch

import backproject_oracle as BO
import forward_project_oracle as FO
import nonconfocal_oracle as NO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRIDS = [(1, 1, 1), (9, 5, 13), (17, 8, 3)]
MEAS = [1, 3, 257]
NRS = [1, 2, 40]
R0S = [0.0, 0.3]
CASES = [(g, nm, nr, r0) for g in GRIDS for nm in MEAS for nr in NRS for r0 in R0S]
DMIN = 0.05          # parity of the negative powers: pairs closer than this to a laser spot or sensed point are left out


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"g{'x'.join(map(str, p[0]))}-m{p[1]}-nr{p[2]}-r{p[3]}")
def case(request):
    return NO.problem(*request.param)


@pytest.fixture(scope="module")
def mid():
    """The case most tests share: 9 x 5 x 13 voxels, 257 measurements, 40 bins, r0 = 0.3 (dr = 0.015)."""
    return NO.problem((9, 5, 13), 257, 40, 0.3)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _grid(tabs):
    from nlosgr.voxelize import VoxelGrid
    return VoxelGrid(tables=[torch.from_numpy(np.ascontiguousarray(t)) for t in tabs])


def _bp(c, power=0, lasers="own", rows=None, sensors=None, grid=None, **kw):
    from nlosgr.backproject import backproject
    lasers = c["lasers"] if isinstance(lasers, str) else lasers
    return backproject(_dev(c["rows"] if rows is None else rows), _dev(c["sensors"] if sensors is None else sensors),
                       grid or _grid(c["tabs"]), c["r0"], c["dr"], power=power,
                       lasers=None if lasers is None else _dev(lasers), **kw)


def _fp(c, power=0, lasers="own", vol=None, grid=None, **kw):
    from nlosgr.forward_project import forward_project
    lasers = c["lasers"] if isinstance(lasers, str) else lasers
    return forward_project(_dev(c["vol"] if vol is None else vol), _dev(c["sensors"]), grid or _grid(c["tabs"]), c["r0"],
                           c["dr"], c["nr"], power=power, lasers=None if lasers is None else _dev(lasers), **kw)


def _bp64(c, power, lasers=None, rows=None, **kw):
    own = lasers is None
    return NO.backproject64(c["rows"] if rows is None else rows, c["sensors"], c["lasers"] if own else lasers, *c["tabs"],
                            *NO.window(c), power, d=c["d"] if own else None, **kw)


def _fp64(c, power, lasers=None, vol=None, dmin=None, **kw):
    own = lasers is None
    return NO.forward64(c["vol"] if vol is None else vol, c["sensors"], c["lasers"] if own else lasers, *c["tabs"],
                        *NO.window(c), c["nr"], power, dmin=None if dmin is None else np.float32(dmin),
                        d=c["d"] if own else None, **kw)


def _share(err, B):
    m = B > 0
    return float((err[m] / B[m]).max()) if m.any() else 0.0


def _np64(t):
    return t.cpu().numpy().astype(np.float64)


def test_parity_within_the_bound(case):
    bw, fw = [], []
    for power in range(5):
        ref, B = _bp64(case, power)
        got = _np64(_bp(case, power))
        assert got.shape == case["shape"] and np.isfinite(got).all()
        err = np.abs(got - ref)
        bw.append(_share(err, B))
        assert np.all(err <= B), ("back-projection", power, bw[-1])
    for power in (0, 1, 2, 3, 4, -1, -2, -3, -4):
        ref, B = _fp64(case, power, dmin=DMIN)
        got = _np64(_fp(case, power, dmin=DMIN))
        assert got.shape == (case["nmeas"], case["nr"]) and np.isfinite(got).all()
        err = np.abs(got - ref)
        fw.append(_share(err, B))
        assert np.all(err <= B), ("forward projection", power, fw[-1])
    print(f"grid {case['shape']} measurements {case['nmeas']} nr {case['nr']} r0 {case['r0']}: worst e/B back-projection "
          f"powers 0..4: " + " ".join(f"{w:.4f}" for w in bw) + "; forward 0..4, -1..-4: "
          + " ".join(f"{w:.4f}" for w in fw))


@pytest.mark.parametrize("shape,nmeas", [((9, 5, 13), 257), ((16, 16, 16), 3)])
def test_lasers_on_the_sensed_points_give_the_confocal_result(shape, nmeas):
    """lasers = walls.clone(): g == d and m == d*d exactly, so the even powers are the confocal kernels' bits; the
    odd powers (sqrt(d*d) against d) stay within the bound."""
    c = NO.problem(shape, nmeas, 40, 0.3)
    same = c["sensors"].copy()
    for power in (0, 2, 4):
        assert torch.equal(_bp(c, power, lasers=same), _bp(c, power, lasers=None)), power
    for power in (1, 3):
        ref, B = _bp64(c, power, lasers=same)
        err = np.abs(_np64(_bp(c, power, lasers=same)) - ref)
        print(f"lasers == sensors, grid {shape}, power {power}: worst e/B {_share(err, B):.4f}")
        assert np.all(err <= B)
    assert c["r0"] == 0.3 and abs(c["dr"] - 0.015) < 1e-12 and c["nr"] == 40
    dmin = c["r0"] - 1.5 * c["dr"]
    r0, inv_dr = NO.window(c)
    vmax, nvox = float(np.abs(c["vol"]).max()), c["vol"].size
    for power in (0, 2, -2, 4, -4):
        assert NO.quantum(vmax, r0, inv_dr, power, 40, nvox, dmin=np.float32(dmin)) == \
            FO.quantum(vmax, r0, inv_dr, power, 40, nvox), power
        got = _fp(c, power, lasers=same, dmin=dmin)
        assert got.any() and torch.equal(got, _fp(c, power, lasers=None)), power


def test_one_laser_equals_the_expanded_list(mid):
    one = mid["lasers"][:1]
    many = np.ascontiguousarray(np.broadcast_to(one, (mid["nmeas"], 3)))
    for power in (0, 3, -2):
        if power >= 0:
            a = _bp(mid, power, lasers=one)
            assert a.any() and torch.equal(a, _bp(mid, power, lasers=many)), power
        r = _fp(mid, power, lasers=one, dmin=DMIN)
        assert r.any() and torch.equal(r, _fp(mid, power, lasers=many, dmin=DMIN)), power
    ref, B = _bp64(mid, 3, lasers=one)
    assert np.all(np.abs(_np64(_bp(mid, 3, lasers=one)) - ref) <= B)
    ref, B = _fp64(mid, -2, lasers=one, dmin=DMIN)
    assert np.all(np.abs(_np64(_fp(mid, -2, lasers=one, dmin=DMIN)) - ref) <= B)


def test_forward_is_repeatable_and_independent_of_the_split():
    few = NO.problem((19, 10, 21), 3, 40, 0.3)
    many = NO.problem((16, 16, 16), 257, 40, 0.3)
    for c in (few, many):
        grid = _grid(c["tabs"])
        for lasers in (c["lasers"], c["lasers"][:1]):
            for power in (0, 3, -2):
                full = _fp(c, power, lasers=lasers, grid=grid, dmin=DMIN)
                assert full.any() and torch.equal(full, _fp(c, power, lasers=lasers, grid=grid, dmin=DMIN))
                for ns in (1, 2, 7):
                    assert torch.equal(full, _fp(c, power, lasers=lasers, grid=grid, dmin=DMIN, nsplit=ns)), (power, ns)
    c = few
    assert torch.equal(_bp(c, 3), _bp(c, 3)) and torch.equal(_bp(c, 3, lasers=c["lasers"][:1]), _bp(c, 3, lasers=c["lasers"][:1]))


def test_dmin_leaves_out_the_pairs_next_to_a_laser(mid):
    """One laser exactly on voxel (4, 2, 6): its weight m^(-p/2) is infinite there.  With dmin = 0.02 the rows are
    finite and within the bound of the oracle that skips the same pairs; without a dmin the Python layer has no
    bound to offer and raises."""
    from nlosgr.forward_project import forward_project
    tabs = mid["tabs"]
    laser = np.array([[tabs[0][4], tabs[1][2], tabs[2][6]]], dtype=np.float32)
    ds, dl = NO.distances64(mid["sensors"], laser, *tabs)
    assert dl.min() == 0.0 and np.sort(dl[:, 0])[1] > 0.02
    for power in (-4, -1):
        ref, B = _fp64(mid, power, lasers=laser, dmin=0.02)
        got = _np64(_fp(mid, power, lasers=laser, dmin=0.02))
        err = np.abs(got - ref)
        print(f"dmin 0.02, laser on a voxel, power {power}: worst e/B {_share(err, B):.4f}")
        assert np.isfinite(got).all() and got.any() and np.all(err <= B)
    with pytest.raises(ValueError, match="dmin"):
        _fp(mid, -4, lasers=laser)
    # a wall in front of the grid: the default is the smallest distance from a wall point to the grid's box
    S = BO.SCENE
    stabs = BO.linspace_tables(S["position"], S["size"], 5)
    walls = _dev(BO.relay_wall(4, 4))
    vol = torch.ones(5, 5, 5, device=DEV)
    a = forward_project(vol, walls, _grid(stabs), 0.2, 0.01, 80, power=-4, lasers=walls[:1])
    b = forward_project(vol, walls, _grid(stabs), 0.2, 0.01, 80, power=-4, lasers=walls[:1], dmin=0.25)
    assert a.any() and torch.equal(a, b)


def test_adjoint_on_the_device(mid):
    """|<A v, h> - <v, A^T h>| (float64 inner products of the fp32 outputs) within what the two bounds allow."""
    c = mid
    h = c["rows"]
    for power in (0, 2, 4):
        _, Bf = _fp64(c, power)
        _, Bb = _bp64(c, power)
        Av, Ath = _np64(_fp(c, power)), _np64(_bp(c, power))
        lhs, rhs = float((Av * h).sum()), float((c["vol"].astype(np.float64) * Ath).sum())
        tol = float((Bf * np.abs(h)).sum() + (np.abs(c["vol"]) * Bb).sum())
        print(f"non-confocal adjoint power {power}: <Av,h> {lhs:.9g} <v,Ath> {rhs:.9g} difference / allowed "
              f"{abs(lhs - rhs) / tol:.4f}")
        assert abs(lhs - rhs) <= tol


def test_accumulate(mid):
    c = mid
    grid = _grid(c["tabs"])
    for power in (0, 2):
        ref, B = _bp64(c, power)
        one = _bp(c, power, grid=grid)
        acc = _bp(c, power, rows=c["rows"][:128], sensors=c["sensors"][:128], lasers=c["lasers"][:128], grid=grid)
        same = _bp(c, power, rows=c["rows"][128:], sensors=c["sensors"][128:], lasers=c["lasers"][128:], grid=grid,
                   out=acc, accumulate=True)
        assert same is acc
        o = one.cpu().numpy()
        ulp = np.spacing(np.abs(o)).astype(np.float64)
        diff = np.abs(_np64(acc) - o.astype(np.float64))
        print(f"accumulate back-projection power {power}: worst |halves - one| / (B + ulp) {float((diff / (B + ulp)).max()):.4f}")
        assert np.all(diff <= B + ulp)
    lo, hi = grid.slice(ix=(0, 4)), grid.slice(ix=(4, 9))
    for power in (0, -4):
        ref, B = _fp64(c, power, dmin=DMIN)
        one = _fp(c, power, grid=grid, dmin=DMIN)
        acc = _fp(c, power, vol=c["vol"][:4], grid=lo, dmin=DMIN)
        same = _fp(c, power, vol=c["vol"][4:], grid=hi, dmin=DMIN, out=acc, accumulate=True)
        assert same is acc
        o = one.cpu().numpy()
        ulp = np.spacing(np.abs(o)).astype(np.float64)
        diff = np.abs(_np64(acc) - o.astype(np.float64))
        print(f"accumulate forward power {power}: worst |halves - one| / (B + ulp) {float((diff / (B + ulp)).max()):.4f}")
        assert np.all(diff <= B + ulp)


@pytest.mark.parametrize("nsplit", [1, 2])
def test_forward_edge_values(nsplit):
    c = NO.problem((9, 5, 13), 3, 40, 0.3)
    zero = np.zeros(c["shape"], dtype=np.float32)
    for lasers in (c["lasers"], c["lasers"][:1]):
        out = torch.full((3, 40), 7.0, device=DEV)
        assert not _fp(c, 0, lasers=lasers, vol=zero, out=out, nsplit=nsplit).any()
        kept = _fp(c, 0, lasers=lasers, vol=zero, out=torch.full((3, 40), 7.0, device=DEV), accumulate=True, nsplit=nsplit)
        assert (kept == 7.0).all()
        for at in ((4, 2, 6), (0, 0, 0)):
            vol = c["vol"].copy()
            vol[at] = np.nan
            assert torch.isnan(_fp(c, 1, lasers=lasers, vol=vol, nsplit=nsplit)).all(), at


def test_nan_bin_and_no_measurements(mid):
    """A NaN in bin b of measurement i reaches the voxels whose u_i lies inside (b-1, b+1) and no others (voxels
    within 1e-3 bins of either limit are left out: the fp32 u may fall on either side); no measurements: zero
    fill, untouched with accumulate, and a forward projection that writes nothing."""
    from nlosgr.backproject import backproject
    from nlosgr.forward_project import forward_project
    c = mid
    i, b, m = 130, 17, 1e-3
    rows = c["rows"].copy()
    rows[i, b] = np.nan
    clean = c["rows"].copy()
    clean[i, b] = 0.0
    u = NO.bin_coordinate(c["d"][0][:, i], c["d"][1][:, i], *NO.window(c)).reshape(c["shape"])
    hit, miss = np.abs(u - b) < 1 - m, np.abs(u - b) > 1 + m
    assert hit.sum() >= 10 and miss.sum() >= 10
    got = _bp(c, 1, rows=rows).cpu().numpy()
    assert np.isnan(got[hit]).all() and np.isfinite(got[miss]).all()
    ref, B = _bp64(c, 1, rows=clean)
    assert np.all(np.abs(got[miss].astype(np.float64) - ref[miss]) <= B[miss])
    grid = _grid(c["tabs"])
    none = torch.zeros(0, 3, device=DEV)
    for lasers in (none, torch.zeros(1, 3, device=DEV)):
        z = backproject(torch.zeros(0, 40, device=DEV), none, grid, 0.3, 0.015, lasers=lasers,
                        out=torch.full(c["shape"], 7.0, device=DEV))
        assert not z.any()
        keep = backproject(torch.zeros(0, 40, device=DEV), none, grid, 0.3, 0.015, lasers=lasers,
                           out=torch.full(c["shape"], 7.0, device=DEV), accumulate=True)
        assert (keep == 7.0).all()
        assert forward_project(_dev(c["vol"]), none, grid, 0.3, 0.015, 40, lasers=lasers).shape == (0, 40)


def _scatterer():
    """backproject_oracle.SCENE with one laser spot at (-0.45, 0, 0.45): (rows, walls, laser, tabs)."""
    S = BO.SCENE
    walls = BO.relay_wall(*S["wall"])
    tabs = BO.linspace_tables(S["position"], S["size"], S["res"])
    laser = np.array([[-0.45, 0.0, 0.45]], dtype=np.float32)
    i, j, k = S["voxel"]
    rows, u = NO.scatterer_rows(walls, laser, (tabs[0][i], tabs[1][j], tabs[2][k]), *BO.scene_window(), S["nr"])
    return rows, u, walls, laser, tabs


def test_point_scatterer_peaks_at_its_voxel():
    """The rows of a scatterer at voxel (11, 5, 3) seen from one laser spot: the non-confocal back-projection peaks
    there (float64: 175.8, the next voxel 87.1); the confocal one of the same rows puts the light on spheres
    around the sensed points and peaks at (11, 13, 3), with under 1 % of the peak at the scatterer (0.86)."""
    from nlosgr.backproject import backproject
    S = BO.SCENE
    rows, u, walls, laser, tabs = _scatterer()
    assert 45 <= np.floor(u.min()) and np.floor(u.max()) + 1 <= 73 and np.allclose(rows.sum(axis=1), 1.0, atol=1e-6)
    ref, B = NO.backproject64(rows, walls, laser, *tabs, *BO.scene_window(), 0)
    top = np.sort(ref.reshape(-1))
    assert np.unravel_index(ref.argmax(), ref.shape) == S["voxel"] and abs(top[-1] - 175.8) < 0.05 and abs(top[-2] - 87.1) < 0.05
    grid = _grid(tabs)
    got = backproject(_dev(rows), _dev(walls), grid, S["r0"], S["dr"], lasers=_dev(laser)).cpu().numpy()
    assert np.unravel_index(got.argmax(), got.shape) == S["voxel"]
    assert np.all(np.abs(got.astype(np.float64) - ref) <= B)
    conf = backproject(_dev(rows), _dev(walls), grid, S["r0"], S["dr"]).cpu().numpy()
    assert np.unravel_index(conf.argmax(), conf.shape) == (11, 13, 3)
    assert conf[S["voxel"]] < 0.01 * got.max()


def test_landweber_with_lasers():
    """A phantom of three voxels seen by 64 measurements from one laser spot, power 0, 20 iterations on its own
    forward projection: the criterion of test_landweber_on_the_device (the objective falls, to at most 0.6 of its
    first value)."""
    from nlosgr.forward_project import forward_project, landweber
    c = NO.problem((9, 5, 13), 64, 40, 0.3)
    grid = _grid(c["tabs"])
    phantom = np.zeros(c["shape"], dtype=np.float32)
    phantom[4, 2, 6], phantom[2, 3, 9], phantom[6, 1, 3] = 1.0, 0.5, 2.0
    sensors, laser = _dev(c["sensors"]), _dev(c["lasers"][:1])
    rows = forward_project(_dev(phantom), sensors, grid, c["r0"], c["dr"], 40, lasers=laser)
    vol, obj = landweber(rows, sensors, grid, c["r0"], c["dr"], iterations=20, lasers=laser)
    o = obj.cpu().numpy()
    print(f"landweber with one laser: objective {o[0]:.4g} -> {o[-1]:.4g} ({o[-1] / o[0]:.3f})")
    assert vol.shape == c["shape"] and (vol >= 0).all() and o[0] > 0
    assert np.all(np.diff(o) <= 0), o
    assert o[-1] <= 0.6 * o[0], o


def test_command_lines_on_a_non_confocal_capture(tmp_path):
    """A capture written with laserGridPositions (the rows are forward_project(power=-4, lasers=) of a one-voxel
    phantom): python -m nlosgr.backproject and python -m nlosgr.forward_project (their main(), in process) read
    the laser spot, write the documented keys, and their volumes peak at the phantom."""
    from nlosgr import backproject as bpm, forward_project as fpm
    from nlosgr.data import make_data_kwargs, save_zaragoza
    S = BO.SCENE
    _, _, walls, laser, tabs = _scatterer()
    phantom = np.zeros((17, 17, 17), dtype=np.float32)
    phantom[S["voxel"]] = 1.0
    rows = fpm.forward_project(_dev(phantom), _dev(walls), _grid(tabs), S["r0"], S["dr"], S["nr"], power=-4,
                               lasers=_dev(laser)).cpu().numpy()
    assert rows.any()
    data = np.zeros((100, 16, 16), dtype=np.float32)
    data[20:100] = rows.T.reshape(80, 16, 16)
    cap, out, lw = str(tmp_path / "cap.mat"), str(tmp_path / "bp.npz"), str(tmp_path / "lw.npz")
    save_zaragoza(cap, data, walls.T, S["position"], S["size"], 0.01, 1.0, laser_grid_positions=laser.T)
    dk, *_ = make_data_kwargs(cap, DEV, shuffle=False)
    assert tuple(dk["laser_grid_positions"].shape) == (3, 1)
    keys = ["density", "albedo", "front", "depth", "xs", "ys", "zs", "cam"]
    bpm.main([cap, "--resolution", "17", "--start", "20", "--end", "100", "--filter", "none", "--out", out])
    z = np.load(out)
    assert sorted(z.files) == sorted(keys)
    want = bpm.backproject(_dev(rows), _dev(walls), _grid(tabs), 20 * 0.01, 0.01, lasers=_dev(laser)).clamp_(min=0.0)
    assert np.array_equal(z["density"], want.cpu().numpy())
    assert np.unravel_index(z["density"].argmax(), (17, 17, 17)) == S["voxel"]
    fpm.main([cap, "--resolution", "17", "--start", "20", "--end", "100", "--iterations", "6", "--out", lw])
    z = np.load(lw)
    assert sorted(z.files) == sorted(keys + ["objective"])
    assert z["objective"].shape == (6,) and np.all(np.diff(z["objective"]) < 0)
    assert np.unravel_index(z["density"].argmax(), (17, 17, 17)) == S["voxel"]
    # the same capture shuffled: only the order of the sum changes, and B does not depend on that order
    torch.manual_seed(0)
    dks, *_ = make_data_kwargs(cap, DEV, shuffle=True)
    shuffled = bpm.backproject_capture(dks, 17, 20, 100, filter="none")["volume"].cpu().numpy()
    _, B = NO.backproject64(rows, walls, laser, *tabs, *BO.scene_window(), 0)
    assert np.unravel_index(shuffled.argmax(), (17, 17, 17)) == S["voxel"]
    assert np.all(np.abs(shuffled.astype(np.float64) - np.load(out)["density"]) <= 2 * B)


def test_error_cases():
    from nlosgr.backproject import backproject
    from nlosgr.forward_project import forward_project, landweber, operator_norm
    grid = _grid(NO.tables((4, 4, 4)))
    rows, walls = torch.zeros(5, 8, device=DEV), torch.zeros(5, 3, device=DEV)
    vol = torch.zeros(4, 4, 4, device=DEV)
    ok = torch.zeros(5, 3, device=DEV)
    for bad, exc in ((ok.cpu(), RuntimeError), (ok.double(), RuntimeError), ([[0.0] * 3] * 5, RuntimeError),
                     (torch.zeros(2, 3, device=DEV), ValueError), (torch.zeros(5, 2, device=DEV), ValueError),
                     (torch.zeros(3, device=DEV), ValueError), (torch.zeros(0, 3, device=DEV), ValueError)):
        with pytest.raises(exc):
            backproject(rows, walls, grid, 0.0, 0.01, lasers=bad)
        with pytest.raises(exc):
            forward_project(vol, walls, grid, 0.0, 0.01, 8, lasers=bad)
        with pytest.raises(exc):
            landweber(rows, walls, grid, 0.0, 0.01, lasers=bad, iterations=1)
        with pytest.raises(exc):
            operator_norm(walls, grid, 0.0, 0.01, 8, lasers=bad)
    # lasers on another device than the walls: needs a second GPU, so on a one-GPU machine this case is NOT run
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            backproject(rows, walls, grid, 0.0, 0.01, lasers=ok.to("cuda:1"))
    with pytest.raises(ValueError, match="dmin"):                          # dmin= without lasers=: a forgotten argument
        forward_project(vol, walls, grid, 0.2, 0.01, 8, power=-2, dmin=0.1)
    with pytest.raises(RuntimeError, match="power"):
        backproject(rows, walls, grid, 0.0, 0.01, power=-1, lasers=ok)
    with pytest.raises(RuntimeError, match="dmin"):
        forward_project(vol, walls, grid, 0.0, 0.01, 8, power=-2, lasers=ok, dmin=0.0)
    with pytest.raises(RuntimeError, match="dmin"):
        forward_project(vol, walls, grid, 0.0, 0.01, 8, power=-2, lasers=ok, dmin=float("nan"))
    with pytest.raises(RuntimeError, match="NLOSGR_IRF_MAX_NR"):
        forward_project(vol, walls, grid, 0.0, 0.01, 8193, lasers=ok)
    # the confocal path is what it was: a negative power still needs r0 * inv_dr >= 2 there
    with pytest.raises(RuntimeError, match="r0 \\* inv_dr"):
        forward_project(vol, walls, grid, 0.01, 0.01, 8, power=-4)
