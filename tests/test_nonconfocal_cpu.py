"""Non-confocal voxel operators without a GPU: the fp32 emulation of the back-projection kernel's arithmetic
against the bound the GPU tests use (tests/nonconfocal_oracle.py), the laser spots' way through the capture file
and data_kwargs, the refusal of the confocal-only Gaussian renderer, and the host-side validation of the three
entry points."""
import ctypes

import numpy as np
import pytest
import torch

import backproject_oracle as BO
import nonconfocal_oracle as NO


def test_emulated_fp32_kernel_is_within_the_bound():
    """The kernel's arithmetic restated in numpy fp32 stays far inside B (-s prints the worst share), while a wrong
    bin, a wrong weight and the confocal geometry are each far outside it."""
    c = NO.problem((9, 5, 13), 257, 40, 0.3)
    r0, inv_dr = NO.window(c)
    nr = c["nr"]
    u = NO.bin_coordinate(*c["d"], r0, inv_dr)
    assert (u <= -1).any() and ((u > -1) & (u < 0)).any() and ((u >= 0) & (u <= nr - 1)).any()
    assert ((u > nr - 1) & (u < nr)).any() and (u >= nr).any()
    assert c["d"][0][0, 0] == 0.0                                       # sensed point 0 sits on voxel (0, 0, 0)
    args = (c["rows"], c["sensors"], c["lasers"], *c["tabs"], r0, inv_dr)
    for power in range(5):
        out, B = NO.backproject64(*args, power, d=c["d"])
        e = NO.emulate32(*args, power)
        share = float((np.abs(e.astype(np.float64) - out) / B).max())
        print(f"emulated fp32 non-confocal power {power}: worst e/B {share:.4f}")
        assert share <= 1.0
    out, B = NO.backproject64(*args, 2, d=c["d"])
    far = lambda e: (np.abs(e.astype(np.float64) - out) > 100 * B).any()
    assert far(NO.emulate32(np.roll(c["rows"], 1, axis=1), *args[1:], 2))
    assert far(NO.emulate32(*args, 1))
    assert far(NO.emulate32(c["rows"], c["sensors"], c["sensors"], *args[3:], 2))
    assert far(BO.emulate32(c["rows"], c["sensors"], *args[3:], 2))     # the confocal operator itself


def test_one_laser_is_the_expanded_list_and_the_confocal_limit_on_the_oracle():
    """A self-check of the oracle the GPU tests lean on (no library code runs here): a [1, 3] laser is the repeated
    spot, and lasers == sensors gives the confocal oracles' numbers and quantum."""
    c = NO.problem((9, 5, 13), 3, 40, 0.3)
    r0, inv_dr = NO.window(c)
    one = c["lasers"][:1]
    a, Ba = NO.backproject64(c["rows"], c["sensors"], one, *c["tabs"], r0, inv_dr, 3)
    b, Bb = NO.backproject64(c["rows"], c["sensors"], np.repeat(one, 3, axis=0), *c["tabs"], r0, inv_dr, 3)
    assert np.array_equal(a, b) and np.array_equal(Ba, Bb)
    # lasers == sensors: the confocal oracle's numbers (m^(p/2) against d^p: a rounding of float64 apart)
    for power in (0, 1, 4):
        nc, _ = NO.backproject64(c["rows"], c["sensors"], c["sensors"], *c["tabs"], r0, inv_dr, power)
        co, _ = BO.backproject64(c["rows"], c["sensors"], *c["tabs"], r0, inv_dr, power)
        np.testing.assert_allclose(nc, co, rtol=1e-12, atol=1e-12)
    import forward_project_oracle as FO
    for power in (0, 3, -4):
        nc, _ = NO.forward64(c["vol"], c["sensors"], c["sensors"], *c["tabs"], r0, inv_dr, 40, power, dmin=1e-3)
        co, _ = FO.forward64(c["vol"], c["sensors"], *c["tabs"], r0, inv_dr, 40, power)
        np.testing.assert_allclose(nc, co, rtol=1e-12, atol=1e-12)
    assert NO.quantum(1.0, r0, inv_dr, -4, 40, 585, dmin=np.float32(c["r0"] - 1.5 * c["dr"])) == \
        FO.quantum(1.0, r0, inv_dr, -4, 40, 585)


def _capture(tmp_path, lasers, name="cap.mat", H=3, W=4, T=6):
    from nlosgr.data import save_zaragoza
    g = np.random.default_rng(5)
    data = g.random((T, H, W)).astype(np.float32)
    sensors = g.random((3, H * W)).astype(np.float32)
    path = str(tmp_path / name)
    save_zaragoza(path, data, sensors, (0.0, 0.5, 0.0), 0.5, 0.01, 1.0, laser_grid_positions=lasers)
    return path, data, sensors


def test_lasers_round_trip_through_the_capture_file(tmp_path):
    from nlosgr.data import load_lasers, make_data_kwargs, save_zaragoza
    g = np.random.default_rng(6)
    per = g.random((3, 12)).astype(np.float32)
    one = g.random((3, 1)).astype(np.float32)
    for lasers in (per, one):
        path, data, sensors = _capture(tmp_path, lasers)
        assert np.array_equal(load_lasers(path), lasers)
        dk, *_ = make_data_kwargs(path, "cpu", shuffle=False)
        assert torch.equal(dk["laser_grid_positions"], torch.from_numpy(lasers))
        torch.manual_seed(3)
        dk, nd, pos, index = make_data_kwargs(path, "cpu", shuffle=True)
        idx = index.long().numpy()
        assert sorted(idx.tolist()) == list(range(12)) and idx.tolist() != list(range(12))
        assert np.array_equal(pos.numpy(), sensors[:, idx])
        want = lasers[:, idx] if lasers.shape[1] > 1 else lasers   # column v: the laser of measurement index[v]
        assert np.array_equal(dk["laser_grid_positions"].numpy(), want)
    plain, *_ = _capture(tmp_path, None, "plain.mat")
    assert load_lasers(plain) is None
    dk, *_ = make_data_kwargs(plain, "cpu", shuffle=False)
    assert sorted(dk) == sorted(["nlos_data", "index", "camera_grid_positions", "camera_grid_size", "volume_position",
                                 "volume_size", "volume_box_point", "deltaT", "c", "pmin", "pmax"])
    with pytest.raises(ValueError):
        save_zaragoza(str(tmp_path / "bad.mat"), np.zeros((6, 3, 4), np.float32), np.zeros((3, 12)), (0, 0.5, 0), 0.5,
                      0.01, 1.0, laser_grid_positions=np.zeros((3, 5)))


def test_lasers_and_irf_travel_in_the_same_file(tmp_path):
    """A measured non-confocal capture carries both optional parts: neither pushes the other out of the file."""
    from nlosgr.data import load_irf, load_lasers, make_data_kwargs, save_zaragoza, volume_geometry
    from nlosgr.irf import IRF
    g = np.random.default_rng(8)
    irf = IRF(np.array([0.25, 0.5, 0.25]), 1, 0.125)
    for lasers in (g.random((3, 12)).astype(np.float32), g.random((3, 1)).astype(np.float32)):
        path = str(tmp_path / f"both{lasers.shape[1]}.mat")
        save_zaragoza(path, g.random((6, 3, 4)).astype(np.float32), g.random((3, 12)).astype(np.float32), (0.0, 0.5, 0.0),
                      0.5, 0.01, 1.0, irf=irf, laser_grid_positions=lasers)
        assert np.array_equal(load_lasers(path), lasers)
        got = load_irf(path)
        assert torch.equal(got.taps, irf.taps) and got.center == 1 and got.background == 0.125
        dk, *_ = make_data_kwargs(path, "cpu", shuffle=False)
        assert torch.equal(dk["laser_grid_positions"], torch.from_numpy(lasers)) and torch.equal(dk["irf"].taps, irf.taps)
        with pytest.raises(NotImplementedError, match="confocal only"):
            volume_geometry(dk, 4, 1, 5)


def test_a_mis_shaped_laser_field_is_refused(tmp_path):
    """[n, 3] in place of [3, n] (or any other shape) raises: a reshape would scramble the spots silently."""
    import scipy.io
    from nlosgr.data import load_lasers
    path, data, sensors = _capture(tmp_path, None, "plain.mat")
    m = {k: v for k, v in scipy.io.loadmat(path).items() if not k.startswith("__")}
    for bad in (np.zeros((12, 3), np.float32), np.zeros((3, 5), np.float32), np.zeros((36,), np.float32)):
        scipy.io.savemat(str(tmp_path / "bad.mat"), dict(m, laserGridPositions=bad))
        with pytest.raises(ValueError, match="laserGridPositions"):
            load_lasers(str(tmp_path / "bad.mat"))


def test_the_gaussian_renderer_refuses_a_non_confocal_capture(tmp_path):
    from nlosgr.data import make_data_kwargs, volume_geometry
    g = np.random.default_rng(7)
    path, data, sensors = _capture(tmp_path, g.random((3, 12)).astype(np.float32))
    dk, *_ = make_data_kwargs(path, "cpu", shuffle=False)
    with pytest.raises(NotImplementedError, match="confocal only"):
        volume_geometry(dk, 4, 1, 5)
    one, *_ = _capture(tmp_path, g.random((3, 1)).astype(np.float32), "one.mat")
    dk, *_ = make_data_kwargs(one, "cpu", shuffle=False)
    with pytest.raises(NotImplementedError, match="confocal only"):
        volume_geometry(dk, 4, 1, 5)
    same, *_ = _capture(tmp_path, sensors, "same.mat")                # lasers == sensors: a confocal capture
    torch.manual_seed(4)
    dk, *_ = make_data_kwargs(same, "cpu", shuffle=True)
    geo = volume_geometry(dk, 4, 1, 5)
    plain, *_ = _capture(tmp_path, None, "plain.mat")
    torch.manual_seed(4)
    dk0, *_ = make_data_kwargs(plain, "cpu", shuffle=True)
    geo0 = volume_geometry(dk0, 4, 1, 5)
    assert geo.nwall == 12 and torch.equal(geo.wall, geo0.wall) and torch.equal(geo.r, geo0.r)


def test_entry_points_validate_on_the_host():
    """The three entry points check their arguments before any launch and report through nlosgr_last_error (no
    GPU; the fake non-null pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    for name in ("nlosgr_backproject_nc", "nlosgr_forward_project_nc_workspace_bytes", "nlosgr_forward_project_nc"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    fake = ctypes.c_void_p(4096)
    V = lambda nx=8, ny=8, nz=8, p=fake: _lib.VoxelGrid(nx, ny, nz, p, p, p)
    err = lib.nlosgr_last_error

    BOpt = lambda r0=0.2, inv=100.0, power=0, acc=0: _lib.BackprojectOpts(r0, inv, power, acc)

    def bp(rows=fake, sensors=fake, lasers=fake, nlaser=4, nmeas=4, nr=16, v=None, o=None, out=fake, novg=False,
           noopt=False):
        v, o = v or V(), o or BOpt()
        return lib.nlosgr_backproject_nc(rows, sensors, lasers, nlaser, nmeas, nr, None if novg else ctypes.byref(v),
                                         None if noopt else ctypes.byref(o), out, None)

    for nl in (0, 2, 3, 5, -1):
        assert bp(nlaser=nl) == 1 and b"nlaser" in err(), nl
    assert bp(lasers=None) == 1 and b"lasers" in err()
    assert bp(lasers=None, nlaser=1) == 1 and b"lasers" in err()
    for bad in (dict(nx=0), dict(nz=-2), dict(ny=1025)):
        assert bp(v=V(**bad)) == 1 and b"1..1024" in err(), bad
    assert bp(nr=0) == 1 and b"nr" in err()
    assert bp(nmeas=-1, nlaser=1) == 1 and b"nmeas" in err()
    for p in (-1, 5, 100):
        assert bp(o=BOpt(power=p)) == 1 and b"power" in err(), p
    for inv in (0.0, -3.0, float("inf"), float("nan")):
        assert bp(o=BOpt(inv=inv)) == 1 and b"inv_dr" in err(), inv
    assert bp(o=BOpt(r0=float("nan"))) == 1 and b"r0" in err()
    assert bp(novg=True) == 1 and bp(noopt=True) == 1 and b"null" in err()
    assert bp(v=V(p=None)) == 1 and b"table" in err()
    assert bp(out=None) == 1 and b"output" in err()
    assert bp(rows=None) == 1 and b"rows" in err()
    assert bp(sensors=None) == 1 and b"sensors" in err()

    FOpt = lambda r0=0.2, inv=100.0, power=0, acc=0, ns=0: _lib.ForwardProjectOpts(r0, inv, power, acc, ns)

    def size(nlaser=4, nmeas=4, nr=16, v=None, o=None, dmin=0.0):
        v, o = v or V(), o or FOpt()
        return lib.nlosgr_forward_project_nc_workspace_bytes(nlaser, nmeas, nr, ctypes.byref(v), ctypes.byref(o), dmin)

    def fp(vol=fake, sensors=fake, lasers=fake, nlaser=4, nmeas=4, nr=16, v=None, o=None, dmin=0.0, ws=fake, out=fake):
        v, o = v or V(), o or FOpt()
        return lib.nlosgr_forward_project_nc(vol, sensors, lasers, nlaser, nmeas, nr, ctypes.byref(v), ctypes.byref(o),
                                             dmin, ws, out, None)

    assert size() == 256 and size(nlaser=1) == 256                      # 512 voxels: one split, the header alone
    assert size(v=V(16, 16, 16)) == 256 + 8 * 4 * 16                    # four splits: the int64 rows as well
    assert size(v=V(16, 16, 16), o=FOpt(ns=1)) == 256
    assert size(nmeas=0, nlaser=1) == 256 and fp(nmeas=0, nlaser=1, sensors=None, lasers=None, out=None) == 0
    for nl in (0, 2, 5):
        assert size(nlaser=nl) == 0 and b"nlaser" in err(), nl
        assert fp(nlaser=nl) == 1 and b"nlaser" in err(), nl
    assert fp(lasers=None) == 1 and b"lasers" in err()
    assert fp(sensors=None) == 1 and b"sensors" in err()
    for dmin in (0.0, -1.0, float("nan"), float("inf")):
        for p in (-1, -4):
            assert size(o=FOpt(power=p), dmin=dmin) == 0 and b"dmin" in err(), (p, dmin)
            assert fp(o=FOpt(power=p), dmin=dmin) == 1 and b"dmin" in err(), (p, dmin)
        assert size(o=FOpt(power=2), dmin=dmin) > 0                     # ignored for power >= 0
    assert size(o=FOpt(r0=0.0, power=-4), dmin=0.01) > 0                # no r0 * inv_dr >= 2 rule on this path
    for p in (-5, 5):
        assert size(o=FOpt(power=p), dmin=0.1) == 0 and b"power" in err(), p
    assert size(nr=8193) == 0 and b"NLOSGR_IRF_MAX_NR" in err()
    assert fp(nr=8193) == 3 and b"NLOSGR_IRF_MAX_NR" in err()
    assert size(o=FOpt(ns=-1)) == 0 and b"nsplit" in err()
    assert fp(vol=None) == 1 and fp(ws=None) == 1 and fp(out=None) == 1
    assert lib.nlosgr_abi_version() == 13


def test_python_surface_refuses_cpu_tensors():
    from nlosgr.backproject import backproject
    from nlosgr.forward_project import forward_project
    from nlosgr.voxelize import VoxelGrid
    grid = VoxelGrid((0.0, 0.5, 0.0), 0.5, 4)
    with pytest.raises(RuntimeError):
        backproject(torch.zeros(3, 8), torch.zeros(3, 3), grid, 0.0, 0.01, lasers=torch.zeros(3, 3))
    with pytest.raises(RuntimeError):
        forward_project(torch.zeros(4, 4, 4), torch.zeros(3, 3), grid, 0.0, 0.01, 8, lasers=torch.zeros(1, 3))
