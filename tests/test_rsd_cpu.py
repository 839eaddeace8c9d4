"""The fast phasor field without a GPU: the float64 oracle (tests/rsd_oracle.py) composes (its staged form with numpy
FFTs equals the direct sum), means what include/nlosgr.h says (the direct sum equals a time-domain evaluation with the
untruncated wavelet to the band-truncation level) and puts point scatterers at their voxel, confocal and with one
laser spot; rsd_band and rsd_nt; the host-side validation of the four new entry points; the Python surface."""
import ctypes
import math

import numpy as np
import pytest
import torch

import fk_oracle as FO
import rsd_oracle as RO
from nlosgr import rsd as R


def test_library_carries_the_entry_points():
    from nlosgr import _lib
    lib = _lib.load()
    for name in ("nlosgr_rsd_load", "nlosgr_rsd_kernel", "nlosgr_rsd_apply", "nlosgr_rsd_gather"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.nlosgr_abi_version() == 13


def test_entry_points_validate_on_the_host():
    """Every check runs before any launch and reports through nlosgr_last_error (no GPU; the fake non-null
    pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    fake, fake2 = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    err = lib.nlosgr_last_error

    def load(spec=fake, perm=None, coef=fake, H=4, W=6, Nt=64, q_lo=3, nq=11, sm=6, sn=1, pw=fake2):
        return lib.nlosgr_rsd_load(spec, perm, coef, H, W, Nt, q_lo, nq, sm, sn, pw, None)

    def kernel(ys=fake, ny=5, j0=0, nj=5, y0=0.0, H=4, W=6, sx=0.1, sz=0.1, dr=0.02, Nt=64, q_lo=3, nq=11, power=0,
               laser=0, K=fake2):
        return lib.nlosgr_rsd_kernel(ys, ny, j0, nj, y0, H, W, sx, sz, dr, Nt, q_lo, nq, power, laser, K, None)

    def apply(kf=fake2, pf=fake, nj=5, nq=11, H=4, W=6, out=fake2):
        return lib.nlosgr_rsd_apply(kf, pf, nj, nq, H, W, out, None)

    def gather(field=fake2, H=4, W=6, nq=11, q_lo=3, Nt=64, dr=0.02, power=0, xs=fake, ys=fake, zs=fake, ny=5, j0=0,
               nj=5, laser=1, l=(0.1, 0.0, 0.2), planes=fake, mag=fake):
        return lib.nlosgr_rsd_gather(field, H, W, nq, q_lo, Nt, dr, power, xs, ys, zs, ny, j0, nj, laser, *l, planes,
                                     mag, None)

    for fn in (load, kernel, apply, gather):
        for bad in (dict(H=0), dict(W=-1), dict(H=1025), dict(W=1025)):
            assert fn(**bad) == 1 and b"1..1024" in err(), (fn.__name__, bad)
    for fn in (kernel, gather):
        for bad in (dict(ny=0, nj=0), dict(ny=1025, nj=1025)):
            assert fn(**bad) == 1 and b"ny must be in 1..1024" in err(), (fn.__name__, bad)
        for bad in (dict(j0=-1), dict(nj=0), dict(j0=1, nj=5), dict(j0=5, nj=1)):
            assert fn(**bad) == 1 and b"depth planes" in err(), (fn.__name__, bad)
        for p in (-1, 5, 100):
            assert fn(power=p) == 1 and b"power" in err(), (fn.__name__, p)
        for dr in (0.0, -0.01, float("inf"), float("nan")):
            assert fn(dr=dr) == 1 and b"dr" in err(), (fn.__name__, dr)
    for bad in (dict(nj=0), dict(nj=1025)):
        assert apply(**bad) == 1 and b"depth planes" in err(), bad
    for fn in (load, kernel, gather):
        for Nt in (63, 0, -2, 8194, 8193):
            assert fn(Nt=Nt) == 1 and b"Nt" in err(), (fn.__name__, Nt)
        # the band must stay inside [1, Nt/2 - 1] = [1, 31] and hold 1..512 frequencies
        for bad in (dict(q_lo=0), dict(nq=0), dict(q_lo=21, nq=12), dict(q_lo=31, nq=2), dict(Nt=4096, nq=513)):
            assert fn(**bad) == 1 and b"band" in err(), (fn.__name__, bad)
    for bad in (dict(nq=0), dict(nq=513)):
        assert apply(**bad) == 1 and b"band" in err(), bad
    for bad in (dict(sx=0.0), dict(sz=-1.0), dict(sx=float("nan")), dict(sz=float("inf"))):
        assert kernel(**bad) == 1 and b"sx and sz" in err(), bad
    assert kernel(y0=float("nan")) == 1 and b"y0" in err()
    for sm, sn in ((-1, 1), (6, -1), (6, 2), (7, 1), (1, 6)):     # the last lattice point would leave [0, H W)
        assert load(sm=sm, sn=sn) == 1 and b"strides" in err(), (sm, sn)
    # null and misaligned pointers
    assert load(spec=None) == 1 and b"null spectrum" in err()
    assert load(coef=None) == 1 and b"null band" in err()
    assert load(pw=None) == 1 and b"null padded" in err()
    for bad in (dict(spec=ctypes.c_void_p(4100)), dict(coef=ctypes.c_void_p(4100)), dict(pw=ctypes.c_void_p(4100))):
        assert load(**bad) == 1 and b"aligned" in err(), bad
    assert kernel(ys=None) == 1 and b"null depth" in err()
    assert kernel(K=None) == 1 and b"null kernel" in err()
    assert kernel(K=ctypes.c_void_p(4104)) == 1 and b"aligned" in err()
    assert apply(kf=None) == 1 and b"null kernel" in err()
    assert apply(pf=None) == 1 and b"null image" in err()
    assert apply(out=None) == 1 and b"null product" in err()
    for bad in (dict(kf=ctypes.c_void_p((1 << 30) + 8), out=ctypes.c_void_p((1 << 30) + 8)), dict(pf=ctypes.c_void_p(4104))):
        assert apply(**bad) == 1 and b"aligned" in err(), bad
    # aliasing: in place (out == kf) is the documented one; the image spectrum inside the product, or a product that
    # overlaps the kernel spectrum without being it, is refused
    image = 11 * 4 * 4 * 6 * 8
    assert apply(pf=ctypes.c_void_p((1 << 30) + image)) == 1 and b"alias the image" in err()
    assert apply(pf=fake2) == 1 and b"alias the image" in err()
    assert apply(out=ctypes.c_void_p((1 << 30) + image)) == 1 and b"only as a whole" in err()
    assert apply(kf=ctypes.c_void_p((1 << 30) + 5 * image - 16), out=fake2) == 1 and b"only as a whole" in err()
    assert gather(field=None) == 1 and b"null field" in err()
    assert gather(planes=None) == 1 and b"null planes" in err()
    assert gather(field=ctypes.c_void_p(4100)) == 1 and b"aligned" in err()
    assert gather(zs=None) == 1 and b"null coordinate" in err()
    assert gather(l=(float("nan"), 0.0, 0.0)) == 1 and b"laser" in err()


@pytest.mark.parametrize("name", list(RO.DENSE))
def test_band_against_the_oracle(name):
    kw, _ = RO.dense_problem(name)
    for cycles in (4.0, 2.5):
        q_lo, coef = R.rsd_band(kw["wavelength"], kw["dr"], kw["Nt"], kw["r0"], cycles)
        w_lo, want = RO.band64(kw["wavelength"], kw["dr"], kw["Nt"], kw["r0"], cycles)
        assert q_lo == w_lo and coef.dtype == np.complex128 and coef.shape == want.shape
        assert q_lo >= 1 and q_lo + len(coef) - 1 <= kw["Nt"] // 2 - 1
        assert np.abs(coef - want).max() <= 1e-15 * np.abs(want).max()


def test_band_by_hand_and_its_errors():
    # P = 8 bins, Nt = 64: q_0 = 8, sigma_b = 16/3, sigma_q = 64 / (2 pi 16/3) = 1.9099: the band is [3, 13]
    q_lo, coef = R.rsd_band(0.32, 0.02, 64, 0.0)
    assert (q_lo, len(coef)) == (3, 11)
    # (dr is the fp32 0.02, 2^-25 off: the hand figures hold to 1e-7)
    assert abs(coef[5] - 1.0 / 64) < 1e-7 and np.all(coef.imag == 0)           # q = 8 is the centre; r0 = 0: real
    assert abs(abs(coef[0]) * 64 - math.exp(-0.5 * (16 / 3 * 2 * math.pi * 5 / 64) ** 2)) < 1e-7
    # r0 = 3 bins turns bin q by -2 pi q 3 / Nt
    _, shifted = R.rsd_band(0.32, 0.02, 64, 0.06)
    turn = np.angle(shifted / coef) / (2 * np.pi)
    want = -(np.arange(3, 14) * float(np.float32(0.06)) / float(np.float32(0.02))) / 64
    assert np.abs((turn - want + 0.5) % 1.0 - 0.5).max() < 1e-12
    for bad in (dict(wavelength=0.07), dict(cycles=0.0), dict(cycles=-1.0), dict(Nt=63), dict(Nt=8194), dict(r0=-0.1),
                dict(dr=0.0)):
        args = dict(wavelength=0.32, dr=0.02, Nt=64, r0=0.0, cycles=4.0)
        args.update(bad)
        with pytest.raises(ValueError):
            R.rsd_band(**args)
    with pytest.raises(ValueError, match="512"):                               # a short wavelet: a wide band
        R.rsd_band(0.08, 0.02, 8192, 0.0, cycles=0.25)
    with pytest.raises(ValueError, match="no DFT bin"):                        # q_0 = 0.5, sigma_q = 0.064: empty
        R.rsd_band(8 * 0.02 * 2, 0.02, 4, 0.0, cycles=15.0)


def test_nt_bound_by_hand():
    """A 3 x 3 wall of spacing 0.5 (corners at +-0.5) on y = 0, one depth plane at y = 1, dr = 0.01, r0 = 0.2: the
    longest half path is corner to opposite corner, sqrt(1 + 1 + 1) = 1.7320508, t_max = 153.205; the shortest
    conceivable is the depth, t_min = 80 > 0; P = 8 bins, sigma_b = 16/3, ceil(4 sigma_b) = 22.  With nr = 100 the
    bound is 153.205 + 22 + 1 = 176.2 -> 177 -> 180 = 2^2 3^2 5; with nr = 300 it is 300 + 23 = 323 -> 324 = 2^2 3^4;
    with r0 = 1.2 (t_min = -20, t_max = 53.2) and nr = 100 it is 100 + 20 + 23 = 143 -> 144."""
    xs = zs = np.array([-0.5, 0.0, 0.5], dtype=np.float32)
    ys = np.array([1.0], dtype=np.float32)
    assert R.rsd_nt(100, xs, zs, 0.0, ys, 0.2, 0.01, 0.16) == 180
    assert R.rsd_nt(300, xs, zs, 0.0, ys, 0.2, 0.01, 0.16) == 324
    assert R.rsd_nt(100, xs, zs, 0.0, ys, 1.2, 0.01, 0.16) == 144
    # a laser at the wall's corner: the longest half path is (sqrt(3) + sqrt(3)) / 2, the same; one far off lengthens it
    assert R.rsd_nt(100, xs, zs, 0.0, ys, 0.2, 0.01, 0.16, laser=(0.5, 0.0, 0.5)) == 180
    far = R.rsd_nt(100, xs, zs, 0.0, ys, 0.2, 0.01, 0.16, laser=(3.0, 0.0, 0.0))
    u = 0.5 * (math.sqrt(3.0) + math.sqrt(3.5 ** 2 + 1 + 0.25))
    assert far >= (u - 0.2) / 0.01 + 23 and far % 2 == 0 and far < 1.1 * ((u - 0.2) / 0.01 + 23)
    for n in (far, 180, 324, 144):
        while n % 2 == 0:
            n //= 2
        while n % 3 == 0:
            n //= 3
        while n % 5 == 0:
            n //= 5
        assert n == 1
    assert [R._smooth_even(n) for n in (1, 2, 3, 7, 11, 13, 17, 31, 121, 8191)] == [2, 2, 4, 8, 12, 16, 18, 32, 128, 8192]
    with pytest.raises(ValueError, match="8192"):
        R.rsd_nt(100, xs, zs, 0.0, np.array([90.0], dtype=np.float32), 0.2, 0.01, 0.16)


@pytest.mark.parametrize("name", list(RO.DENSE))
def test_oracle_stages_compose_to_the_direct_sum(name):
    kw, laser = RO.dense_problem(name)
    H, W = kw["H"], kw["W"]
    for l in (None, laser):
        for power in (0, 1, 4):
            ref = RO.reconstruct64(**kw, power=power, laser=l)
            got = RO.staged64(**kw, power=power, laser=l)
            assert ref.shape == got.shape == (W, len(kw["ys"]), H)
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            print(f"{name} laser {l is not None} power {power}: staged vs direct sum {err:.2e} of the maximum")
            assert err <= 1e-10
    # a permuted capture with its perm, and the transposed wall order, are the same lattice
    order = np.random.default_rng(1).permutation(H * W)               # shuffled row u holds lattice point order[u]
    base = RO.staged64(**kw)
    assert np.array_equal(RO.staged64(**dict(kw, rows=kw["rows"][order]), perm=np.argsort(order)), base)
    t = np.arange(H * W).reshape(H, W).T.reshape(-1)
    assert np.array_equal(RO.staged64(**dict(kw, rows=kw["rows"][t]), x_along="m"), base)
    # the padding and the entries at offset -H / -W are zero
    sx, sz = RO.spacings(kw["xs"], kw["zs"])
    q_lo, coef = RO.band64(kw["wavelength"], kw["dr"], kw["Nt"], kw["r0"])
    K = RO.kernel64(kw["ys"], kw["y0"], H, W, sx, sz, kw["dr"], kw["Nt"], q_lo, len(coef), 1, False)
    assert not K[:, :, H].any() and not K[:, :, :, W].any() and (K[:, :, :H, :W] != 0).all()
    Pw = RO.load64(np.fft.rfft(kw["rows"].astype(np.float64), n=kw["Nt"], axis=1), H, W, q_lo, coef)
    assert not Pw[:, H:].any() and not Pw[:, :, W:].any() and Pw[:, :H, :W].all()


@pytest.mark.parametrize("name", ["8x8x32", "5x7x17_r3"])
def test_the_direct_sum_means_the_time_domain_phasor_field(name):
    """Meaning: the band-limited direct sum against the rows filtered in time with the untruncated Morlet wavelet at the
    continuous bin coordinate (periodic in Nt), weighted as nonconfocal_oracle / backproject_oracle weigh.  The two
    differ by the band's +-3 sigma_q truncation alone: measured 7.8e-3 to 1.7e-2 of the maximum (the 1-D check of the
    wavelet gave 6e-3 of a row's maximum)."""
    kw, laser = RO.dense_problem(name)
    for l in (None, laser):
        for power in (0, 2):
            ref = RO.timedomain64(**kw, power=power, laser=l)
            got = RO.reconstruct64(**kw, power=power, laser=l)
            level = float(np.abs(got - ref).max() / np.abs(ref).max())
            print(f"{name} laser {l is not None} power {power}: band truncation level {level:.2e} of the maximum")
            assert level < 2e-2


@pytest.mark.parametrize("with_laser", [False, True], ids=["confocal", "one_laser"])
@pytest.mark.parametrize("name", list(FO.SCATTERERS))
def test_oracle_puts_a_point_scatterer_at_its_voxel(name, with_laser):
    """The scenes of the GPU test, known good before they reach a GPU: at a wavelength of three wall spacings the
    oracle's magnitude peaks at the scatterer's voxel, confocal and with one laser spot, 40 to 320 times above the
    median, so the fp32 kernels, held to 2e-5 of the maximum, keep the argmax."""
    kw, laser, voxel = RO.scatterer_problem(name, with_laser)
    c = FO.SCATTERERS[name]
    assert 2.0 <= kw["wavelength"] / c["sx"] <= 4.0 and (kw["rows"].sum(axis=1) > 0).mean() > 0.5
    Nt = R.rsd_nt(c["nr"], kw["xs"], kw["zs"], kw["y0"], kw["ys"], kw["r0"], kw["dr"], kw["wavelength"], 4.0, laser)
    mag = np.abs(RO.staged64(**kw, Nt=Nt, laser=laser))
    at, ratio = RO.argmax3(mag), float(mag.max() / np.median(mag))
    print(f"{name} laser {with_laser}: Nt {Nt}, argmax {at}, peak / median {ratio:.3g}")
    assert at == voxel and ratio >= 20


def test_python_surface_refuses_cpu_tensors_and_bad_shapes():
    rows = torch.zeros(24, 8)
    xs, zs, ys = torch.linspace(-0.25, 0.25, 6), torch.linspace(-0.15, 0.15, 4), torch.tensor([0.3, 0.4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.rsd_reconstruct(rows, 4, 6, xs, zs, 0.0, ys, 0.0, 0.02, 0.32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.rsd_load(torch.zeros(24, 33, dtype=torch.complex64), 4, 6, 3, np.ones(11, dtype=np.complex128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.rsd_kernel(ys, 0.0, 4, 6, 0.1, 0.1, 0.02, 64, 3, 11)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.rsd_apply(torch.zeros(2, 11, 8, 12, dtype=torch.complex64), torch.zeros(11, 8, 12, dtype=torch.complex64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.rsd_gather(torch.zeros(2, 11, 8, 12, dtype=torch.complex64), 3, 64, 0.02, xs, ys, zs)
    with pytest.raises(ValueError):
        R._lattice(0, 6)
    with pytest.raises(ValueError):
        R._lattice(4, 1025)
    with pytest.raises(ValueError):
        R._laser([0.0, 1.0])
    with pytest.raises(ValueError):
        R._chunk(5, 3, 3)
    assert R._chunk(5, 2, None) == (2, 3) and R._laser(None) is None and R._laser(torch.tensor([1.0, 2.0, 3.0])) == [1.0, 2.0, 3.0]
    import nlosgr
    assert nlosgr.rsd_capture is R.rsd_capture and nlosgr.rsd_reconstruct is R.rsd_reconstruct


def test_capture_laser_tells_the_three_kinds_apart():
    walls = torch.tensor(FO.lattice(4, 6, 0.1, 0.1)[2]).t().contiguous()
    assert R.capture_laser({"camera_grid_positions": walls}) is None
    assert R.capture_laser({"camera_grid_positions": walls, "laser_grid_positions": walls.clone()}) is None
    one = torch.tensor([[0.1], [0.0], [-0.2]])
    got = R.capture_laser({"camera_grid_positions": walls, "laser_grid_positions": one})
    assert got == [float(np.float32(0.1)), 0.0, float(np.float32(-0.2))]
    assert R.capture_laser({"camera_grid_positions": walls, "laser_grid_positions": one.expand(3, 24).contiguous()}) == got
    shifted = walls + torch.tensor([[0.1], [0.0], [0.0]])
    with pytest.raises(NotImplementedError, match="nlosgr.phasor"):
        R.capture_laser({"camera_grid_positions": walls, "laser_grid_positions": shifted})


def test_command_line_arguments(capsys):
    a = R.parse_args(["cap.mat", "--start", "20", "--end", "100", "--wavelength", "0.2"])
    assert (a.resolution, a.cycles, a.power, a.out, a.mesh, a.level_frac) == (128, 4.0, 0, "rsd.npz", None, 0.5)
    a = R.parse_args(["cap.mat", "--resolution", "32", "--start", "0", "--end", "64", "--wavelength", "0.25", "--cycles", "5",
                      "--power", "2", "--mesh", "m.ply", "--level-frac", "0.3"])
    assert (a.resolution, a.wavelength, a.cycles, a.power, a.mesh, a.level_frac) == (32, 0.25, 5.0, 2, "m.ply", 0.3)
    for end in ("20", "19"):
        with pytest.raises(SystemExit):
            R.parse_args(["cap.mat", "--start", "20", "--end", end, "--wavelength", "0.2"])
        assert "--end must be greater than --start" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        R.parse_args(["cap.mat", "--start", "20", "--end", "100"])                       # no wavelength
    with pytest.raises(SystemExit):
        R.parse_args(["cap.mat", "--start", "20", "--end", "100", "--wavelength", "0.2", "--power", "5"])


def test_initialiser_needs_a_wavelength_for_rsd():
    from types import SimpleNamespace
    from nlosgr.init import sample_from_backprojection
    args = SimpleNamespace(init_gaussian_num=4, carving_volume_size=5)
    with pytest.raises(ValueError, match="wavelength"):
        sample_from_backprojection(args, {}, method="rsd")
    with pytest.raises(ValueError):
        sample_from_backprojection(args, {}, method="lct")
