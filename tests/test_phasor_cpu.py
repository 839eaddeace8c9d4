"""Phasor-field reconstruction without a GPU: the new entry point's presence and host-side validation, the Morlet
wavelet of nlosgr.phasor.phasor_kernel against a float64 restatement, the point-scatterer condition the GPU argmax
test rests on (on the float64 oracle alone: tests/phasor_oracle.py), and the command line's argument check."""
import ctypes

import numpy as np
import pytest
import torch

import backproject_oracle as BO
import phasor_oracle as PO

WAVELENGTH, CYCLES = 0.16, 4.0       # of the point-scatterer checks: P = 8 bins, 33 taps


def test_library_carries_the_entry_point():
    from nlosgr import _lib
    lib = _lib.load()
    assert hasattr(lib, "nlosgr_backproject_phasor") and "nlosgr_backproject_phasor" in _lib.EXPORTS
    assert lib.nlosgr_abi_version() == 13


def test_entry_point_validates_on_the_host():
    """Every check runs before any launch and reports through nlosgr_last_error (no GPU; the fake non-null
    pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    V = lambda nx=8, ny=8, nz=8, p=fake: _lib.VoxelGrid(nx, ny, nz, p, p, p)
    BOpt = lambda r0=0.2, inv=100.0, power=0, acc=0: _lib.BackprojectOpts(r0, inv, power, acc)
    err = lib.nlosgr_last_error

    def ph(rows=fake, sensors=fake, lasers=fake, nlaser=4, nmeas=4, nr=16, v=None, o=None, planes=fake, mag=fake,
           novg=False, noopt=False):
        v, o = v or V(), o or BOpt()
        return lib.nlosgr_backproject_phasor(rows, sensors, lasers, nlaser, nmeas, nr, None if novg else ctypes.byref(v),
                                             None if noopt else ctypes.byref(o), planes, mag, None)

    assert ph(novg=True) == 1 and b"null" in err()
    assert ph(noopt=True) == 1 and b"null" in err()
    assert ph(planes=None) == 1 and b"planes" in err()
    assert ph(planes=None, mag=None) == 1 and b"planes" in err()
    for p in (-1, 5, 100):
        assert ph(o=BOpt(power=p)) == 1 and b"power" in err(), p
    for nr in (0, -3):
        assert ph(nr=nr) == 1 and b"nr" in err(), nr
    for nl in (0, 2, 3, 5, -1):                                           # lasers given: 1 or nmeas
        assert ph(nlaser=nl) == 1 and b"nlaser" in err(), nl
    for nl in (1, 4, -1):                                                 # confocal: 0
        assert ph(lasers=None, nlaser=nl) == 1 and b"nlaser" in err(), nl
    for inv in (0.0, -3.0, float("inf"), float("nan")):
        assert ph(o=BOpt(inv=inv)) == 1 and b"inv_dr" in err(), inv
    for r0 in (float("nan"), float("inf"), -float("inf")):
        assert ph(o=BOpt(r0=r0)) == 1 and b"r0" in err(), r0
    # what nlosgr_backproject_nc validates besides
    for bad in (dict(nx=0), dict(nz=-2), dict(ny=1025)):
        assert ph(v=V(**bad)) == 1 and b"1..1024" in err(), bad
    assert ph(nmeas=-1, nlaser=1) == 1 and b"nmeas" in err()
    assert ph(v=V(p=None)) == 1 and b"table" in err()
    assert ph(rows=None) == 1 and b"rows" in err()
    assert ph(sensors=None) == 1 and b"sensors" in err()
    assert ph(lasers=None, nlaser=0, sensors=None) == 1 and b"sensors" in err()


def test_phasor_kernel_matches_the_float64_restatement():
    from nlosgr.irf import MAX_TAPS
    from nlosgr.phasor import phasor_kernel
    for wavelength, dr, cycles in ((0.16, 0.01, 4.0), (0.12, 0.01, 5.0), (0.24, 0.01, 3.0), (0.05, 0.00125, 2.5),
                                   (0.04, 0.01, 1.0)):
        kc, ks = phasor_kernel(wavelength, dr, cycles)
        P = wavelength / (2 * dr)
        sigma = cycles * P / 6
        n = int(np.ceil(3 * sigma))
        m = np.arange(-n, n + 1, dtype=np.float64)
        env = np.exp(-m * m / (2 * sigma * sigma))
        env /= env.sum()
        assert len(kc) == len(ks) == 2 * n + 1 and kc.center == ks.center == n
        assert kc.background == 0.0 and ks.background == 0.0
        c, s = kc.taps.numpy().astype(np.float64), ks.taps.numpy().astype(np.float64)
        assert np.abs(c - env * np.cos(2 * np.pi * m / P)).max() <= 1e-7
        assert np.abs(s - env * np.sin(2 * np.pi * m / P)).max() <= 1e-7
        oc, os_, on = PO.kernel64(wavelength, dr, cycles)
        assert on == n and np.abs(c - oc).max() <= 1e-7 and np.abs(s - os_).max() <= 1e-7
        assert abs(env.sum() - 1.0) <= 1e-15
        # |taps| <= env <= 1, so an fp32 tap is within 2^-25 of its float64 value
        assert np.abs(np.hypot(c, s) - env).max() <= 1e-7                 # the modulus is the envelope: sum env = 1
        assert abs(np.hypot(c, s).sum() - 1.0) <= (2 * n + 1) * 1e-7
        assert np.array_equal(c, c[::-1]) and np.array_equal(s, -s[::-1]) and s[n] == 0.0
    assert len(phasor_kernel(0.16, 0.01, 4.0)[0]) == 33
    with pytest.raises(ValueError, match="Nyquist"):
        phasor_kernel(0.039, 0.01)                                        # P = 1.95
    for cycles in (0.0, -1.0):
        with pytest.raises(ValueError, match="cycles"):
            phasor_kernel(0.16, 0.01, cycles)
    with pytest.raises(ValueError, match=str(MAX_TAPS)):
        phasor_kernel(1.0, 0.001, 4.0)                                    # P = 500: 2001 taps
    assert len(phasor_kernel(0.04, 0.01)[0]) == 9                         # P = 2 exactly is allowed


def test_point_scatterer_condition_on_the_oracle():
    """The float64 phasor image of SCENE's point scatterer peaks at its voxel, at least 1.1 x above the
    second-largest voxel (measured: 1.153): the condition that keeps the GPU argmax test meaningful, confocal
    and with the lasers displaced by PO.LASER_SHIFT (1.153)."""
    S = BO.SCENE
    rows, walls, tabs, r0, inv_dr = BO.scatterer_scene()
    rc = PO.rows64(rows, WAVELENGTH, S["dr"], CYCLES)
    assert rc.shape == (256, 80, 2)
    _, _, mag = PO.backproject64(rc, walls, *tabs, r0, inv_dr, 0, want_bound=False)
    at, ratio = PO.peak(mag)
    print(f"confocal scatterer: argmax {at}, peak / second {ratio:.4f}")
    assert at == S["voxel"] and ratio >= 1.1
    rows, sensors, lasers, tabs, r0, inv_dr = PO.nc_scatterer_scene()
    assert abs(float(np.abs(lasers - sensors).max()) - 0.1) < 1e-6      # 1.6 wall-point spacings off the sensors
    rc = PO.rows64(rows, WAVELENGTH, S["dr"], CYCLES)
    _, _, mag = PO.backproject64(rc, sensors, *tabs, r0, inv_dr, 0, lasers=lasers, want_bound=False)
    at, ratio = PO.peak(mag)
    print(f"lasers displaced by {PO.LASER_SHIFT}: argmax {at}, peak / second {ratio:.4f}")
    assert at == S["voxel"] and ratio >= 1.1


def test_command_line_rejects_an_empty_window(capsys):
    from nlosgr.phasor import parse_args
    a = parse_args(["cap.mat", "--start", "20", "--end", "100", "--wavelength", "0.16"])
    assert (a.resolution, a.cycles, a.power, a.out, a.mesh) == (128, 4.0, 0, "ph.npz", None)
    for end in ("20", "19"):
        with pytest.raises(SystemExit):
            parse_args(["cap.mat", "--start", "20", "--end", end, "--wavelength", "0.16"])
        assert "--end must be greater than --start" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["cap.mat", "--start", "20", "--end", "100"])           # --wavelength is required


def test_python_surface_refuses_cpu_tensors():
    from nlosgr.phasor import phasor_backproject
    from nlosgr.voxelize import VoxelGrid
    grid = VoxelGrid((0.0, 0.5, 0.0), 0.5, 4)
    with pytest.raises(RuntimeError):
        phasor_backproject(torch.zeros(3, 8, 2), torch.zeros(3, 3), grid, 0.0, 0.01)
