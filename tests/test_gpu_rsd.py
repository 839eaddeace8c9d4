"""GPU checks of the fast phasor field (include/nlosgr.h nlosgr_rsd_load / _kernel / _apply / _gather,
csrc/nlosgr_rsd.hip, nlosgr/rsd.py) against the float64 oracle of tests/rsd_oracle.py, which starts from the fp32 inputs
the kernels get.  The end-to-end reference is reconstruct64, the direct sum over wall points and band frequencies with
no FFT at all.

Shapes are the smallest at which the kernels can go wrong: 8 x 8 x 32 (Nt 64, four depth planes of unequal spacing);
5 x 7 x 17 with sx != sz, r0 = 3 dr, y0 != 0 and Nt 40 (every extent odd: every tile partial, the zero column b' = -W
falls on the second complex of a 16-byte store, rows of the spectrum that are not 16-byte aligned); 12 x 20 x 48 (Nt
96); 1 x 9 x 16, a single wall row (Nt 32).  The one-laser runs put the spot off the lattice and off the wall's centre.

Tolerances.  End to end (per voxel, as a fraction of the largest |Phi|), the kernel pass alone (per element, as a
fraction of the largest |K|) and the gather pass alone (per voxel, as a fraction of the largest |Phi|; the oracle is
fed the GPU's own fp32 input, so the FFT's error is not charged to a kernel) are held to 4 x the worst value measured
on the MI355X over all cases and options, one digit up (the rule of DESIGN.md's parity tables), and may not exceed
2e-5 of the maximum, the cap the other reconstructions are held to:

    end to end   measured 1.40e-6 (1 x 9 x 16, confocal, power 4)       4 x = 5.61e-6   tolerance 6e-6
    kernel       measured 2.38e-7 (12 x 20 x 48, confocal, power 3)     4 x = 9.53e-7   tolerance 1e-6
    gather       measured 2.15e-7 (12 x 20 x 48, one laser, power 1)    4 x = 8.59e-7   tolerance 9e-7

(load measured 1.58 and apply 1.73 x 2^-24 of the operands' product; one plane per chunk came out bitwise equal to
unchunked; the normalised magnitudes of the scatterer scenes differ from phasor_backproject's by 1.7e-2 to 4.3e-2 of
the maximum, the two definitions' difference.)

load and apply are single complex products (a + i b)(c + i d) formed as re = fma(a, c, -rn(b d)), im = fma(a, d,
rn(b c)): each component carries the rounding of the inner product, 2^-24 |b d| (or |b c|), and of the fma, 2^-24 of
the component, together at most 2 x 2^-24 |x| |y|; the complex error is at most sqrt(2) times that: both are held per
element to 3 x 2^-24 |x| |y|.  mag is within 1 fp32 ulp of float32(sqrt(float64(re)^2 + float64(im)^2)).  Run with -s
for the measured figures."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fk_oracle as FO
import rsd_oracle as RO
from nlosgr import rsd as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP = 2e-5            # of the maximum: no tolerance here may exceed it
TOL_E2E = 6e-6
TOL_KERNEL = 1e-6
TOL_GATHER = 9e-7
TOL_PRODUCT = 3 * 2.0 ** -24
POWERS = (0, 1, 4)

assert TOL_E2E <= CAP and TOL_KERNEL <= CAP and TOL_GATHER <= CAP


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _c(planes):
    p = planes.cpu().numpy().astype(np.float64)
    return p[0] + 1j * p[1]


def _ulps(got, want):
    g, w = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert np.isfinite(g).all() and (g >= 0).all()
    return int(np.abs(g.view(np.int32).astype(np.int64) - w.view(np.int32).astype(np.int64)).max())


def _run(kw, **over):
    a = dict(kw, **over)
    rows = a.pop("rows")
    return R.rsd_reconstruct(_dev(rows) if isinstance(rows, np.ndarray) else rows, a.pop("H"), a.pop("W"), a.pop("xs"),
                             a.pop("zs"), a.pop("y0"), a.pop("ys"), a.pop("r0"), a.pop("dr"), a.pop("wavelength"), **a)


@pytest.fixture(scope="module")
def dense():
    """name -> (kw, laser), built once."""
    return {name: RO.dense_problem(name) for name in RO.DENSE}


def _band(kw):
    q_lo, coef = R.rsd_band(kw["wavelength"], kw["dr"], kw["Nt"], kw["r0"])
    return q_lo, coef, len(coef)


@pytest.mark.parametrize("name", list(RO.DENSE))
def test_end_to_end_against_the_direct_sum(dense, name):
    kw, laser = dense[name]
    shape = (kw["W"], len(kw["ys"]), kw["H"])
    worst = 0.0
    for l in (None, laser):
        for power in POWERS:
            planes, mag = _run(kw, power=power, laser=l)
            assert planes.shape == (2,) + shape and mag.shape == shape
            assert planes.dtype == mag.dtype == torch.float32 and planes.is_contiguous() and mag.is_contiguous()
            ref = RO.reconstruct64(**kw, power=power, laser=l)
            err = float(np.abs(_c(planes) - ref).max() / np.abs(ref).max())
            print(f"{name} laser {l is not None} power {power}: end-to-end error {err:.3e} of the maximum "
                  f"(tolerance {TOL_E2E:g})")
            worst = max(worst, err)
            p = planes.cpu().numpy().astype(np.float64)
            assert _ulps(mag.cpu().numpy(), np.sqrt(p[0] ** 2 + p[1] ** 2).astype(np.float32)) <= 1
    assert worst <= TOL_E2E, (name, worst)


@pytest.mark.parametrize("name", list(RO.DENSE))
def test_load_alone(dense, name):
    kw, _ = dense[name]
    H, W = kw["H"], kw["W"]
    q_lo, coef, nq = _band(kw)
    spec = torch.fft.rfft(_dev(kw["rows"]), n=kw["Nt"])
    assert spec.shape == (H * W, kw["Nt"] // 2 + 1) and spec.dtype == torch.complex64
    out = torch.full((nq, 2 * H, 2 * W), float("nan"), dtype=torch.complex64, device=DEV)
    got = R.rsd_load(spec, H, W, q_lo, coef, out=out)
    assert got.data_ptr() == out.data_ptr()
    g = got.cpu().numpy()
    assert not np.isnan(g.view(np.float32)).any()
    assert not g[:, H:].any() and not g[:, :, W:].any() and g[:, :H, :W].all()           # the padding: exactly zero
    S = spec.cpu().numpy()
    ref = RO.load64(S, H, W, q_lo, coef)
    scale = np.zeros_like(ref, dtype=np.float64)
    scale[:, :H, :W] = (np.abs(S.astype(np.complex128)).reshape(H, W, -1)[:, :, q_lo:q_lo + nq]
                        * np.abs(RO.c64(coef))[None, None, :]).transpose(2, 0, 1)
    rel = np.abs(g.astype(np.complex128) - ref)[:, :H, :W] / scale[:, :H, :W]
    print(f"{name}: load worst error {rel.max() / 2.0 ** -24:.2f} x 2^-24 |coef| |S|")
    assert rel.max() <= TOL_PRODUCT
    # the rows in another order: the same images, bitwise
    order = np.random.default_rng(4).permutation(H * W)
    perm = _dev(np.argsort(order).astype(np.int32))
    assert torch.equal(got, R.rsd_load(spec[_dev(order)].contiguous(), H, W, q_lo, coef, perm=perm))
    strided = torch.empty((nq, 2 * H, 4 * W), dtype=torch.complex64, device=DEV)[:, :, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        R.rsd_load(spec, H, W, q_lo, coef, out=strided)


@pytest.mark.parametrize("name", list(RO.DENSE))
def test_kernel_alone(dense, name):
    kw, _ = dense[name]
    H, W, Nt = kw["H"], kw["W"], kw["Nt"]
    q_lo, _, nq = _band(kw)
    sx, sz = RO.spacings(kw["xs"], kw["zs"])
    ys = _dev(kw["ys"])
    ny = len(kw["ys"])
    worst = 0.0
    for laser in (False, True):
        for power in (0, 1, 3, 4):
            out = torch.full((ny, nq, 2 * H, 2 * W), float("nan"), dtype=torch.complex64, device=DEV)
            got = R.rsd_kernel(ys, kw["y0"], H, W, sx, sz, kw["dr"], Nt, q_lo, nq, power=power, laser=laser, out=out)
            assert got.data_ptr() == out.data_ptr()
            g = got.cpu().numpy()
            assert not np.isnan(g.view(np.float32)).any()
            assert not g[:, :, H].any() and not g[:, :, :, W].any()                       # a' = -H, b' = -W: exactly zero
            ref = RO.kernel64(kw["ys"], kw["y0"], H, W, sx, sz, kw["dr"], Nt, q_lo, nq, power, laser)
            assert (g != 0).sum() == (ref != 0).sum()
            err = float(np.abs(g.astype(np.complex128) - ref).max() / np.abs(ref).max())
            print(f"{name} laser {laser} power {power}: kernel error {err:.3e} of the largest |K| (tolerance {TOL_KERNEL:g})")
            worst = max(worst, err)
    assert worst <= TOL_KERNEL, (name, worst)
    # a chunk of the planes is that block of the whole, bitwise
    if ny >= 3:
        whole = R.rsd_kernel(ys, kw["y0"], H, W, sx, sz, kw["dr"], Nt, q_lo, nq, power=1)
        part = R.rsd_kernel(ys, kw["y0"], H, W, sx, sz, kw["dr"], Nt, q_lo, nq, power=1, j0=1, nj=2)
        assert part.shape[0] == 2 and torch.equal(part, whole[1:3])


@pytest.mark.parametrize("name", list(RO.DENSE))
def test_apply_alone(dense, name):
    kw, _ = dense[name]
    H, W = kw["H"], kw["W"]
    nq, nj = 5, 3
    g = np.random.default_rng(11)
    cplx = lambda *s: (g.standard_normal(s) + 1j * g.standard_normal(s)).astype(np.complex64)
    Kf, Pf = cplx(nj, nq, 2 * H, 2 * W), cplx(nq, 2 * H, 2 * W)
    out = torch.full((nj, nq, 2 * H, 2 * W), float("nan"), dtype=torch.complex64, device=DEV)
    kd = _dev(Kf)
    got = R.rsd_apply(kd, _dev(Pf), out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(kd.cpu(), torch.from_numpy(Kf))
    o = got.cpu().numpy()
    assert not np.isnan(o.view(np.float32)).any()
    rel = np.abs(o.astype(np.complex128) - RO.apply64(Kf, Pf)) / (np.abs(Kf.astype(np.complex128)) * np.abs(Pf.astype(np.complex128))[None])
    print(f"{name}: apply worst error {rel.max() / 2.0 ** -24:.2f} x 2^-24 |Kf| |Pf|")
    assert rel.max() <= TOL_PRODUCT
    inplace = R.rsd_apply(kd, _dev(Pf))
    assert inplace.data_ptr() == kd.data_ptr() and torch.equal(inplace, got)
    with pytest.raises(ValueError):
        R.rsd_apply(kd, _dev(Pf[:4]))
    with pytest.raises(ValueError, match="contiguous"):
        R.rsd_apply(kd, _dev(Pf), out=torch.empty((nj, nq, 2 * H, 4 * W), dtype=torch.complex64, device=DEV)[..., ::2])


@pytest.mark.parametrize("name", list(RO.DENSE))
def test_gather_alone(dense, name):
    kw, laser = dense[name]
    H, W, Nt = kw["H"], kw["W"], kw["Nt"]
    q_lo, _, nq = _band(kw)
    ny = len(kw["ys"])
    xs, ys, zs = _dev(kw["xs"]), _dev(kw["ys"]), _dev(kw["zs"])
    g = np.random.default_rng(9)
    field = (g.standard_normal((ny, nq, 2 * H, 2 * W)) + 1j * g.standard_normal((ny, nq, 2 * H, 2 * W))).astype(np.complex64)
    field[:, :, H:] = field[:, :, :, W:] = np.nan              # nothing outside the corner is read into the result
    worst = 0.0
    for l in (None, laser):
        for power in POWERS:
            planes = torch.full((2, W, ny, H), float("nan"), device=DEV)
            mag = torch.full((W, ny, H), float("nan"), device=DEV)
            got, gm = R.rsd_gather(_dev(field), q_lo, Nt, kw["dr"], xs, ys, zs, power=power, laser=l, out=planes, mag=mag)
            assert got.data_ptr() == planes.data_ptr() and gm.data_ptr() == mag.data_ptr()
            assert torch.isfinite(planes).all() and torch.isfinite(mag).all()
            ref = RO.gather64(field, H, W, q_lo, Nt, kw["dr"], kw["xs"], kw["ys"], kw["zs"], power, l)
            err = float(np.abs(_c(planes) - ref).max() / np.abs(ref).max())
            print(f"{name} laser {l is not None} power {power}: gather error {err:.3e} of the largest |Phi| "
                  f"(tolerance {TOL_GATHER:g})")
            worst = max(worst, err)
            p = planes.cpu().numpy().astype(np.float64)
            assert _ulps(mag.cpu().numpy(), np.sqrt(p[0] ** 2 + p[1] ** 2).astype(np.float32)) <= 1
    assert worst <= TOL_GATHER, (name, worst)
    # a chunk writes its planes and no other
    if ny >= 3:
        full, fm = R.rsd_gather(_dev(field), q_lo, Nt, kw["dr"], xs, ys, zs, power=1, laser=laser)
        planes = torch.full((2, W, ny, H), float("nan"), device=DEV)
        mag = torch.full((W, ny, H), float("nan"), device=DEV)
        R.rsd_gather(_dev(field[1:3]), q_lo, Nt, kw["dr"], xs, ys, zs, power=1, laser=laser, j0=1, out=planes, mag=mag)
        assert torch.equal(planes[:, :, 1:3], full[:, :, 1:3]) and torch.equal(mag[:, 1:3], fm[:, 1:3])
        assert torch.isnan(planes[:, :, 0]).all() and torch.isnan(planes[:, :, 3:]).all() and torch.isnan(mag[:, 0]).all()
    with pytest.raises(ValueError, match="contiguous"):
        R.rsd_gather(_dev(field), q_lo, Nt, kw["dr"], xs, ys, zs, out=torch.empty((2, W, ny, 2 * H), device=DEV)[..., ::2])


@pytest.mark.parametrize("name", ["12x20x48", "5x7x17_r3"])
def test_one_plane_per_chunk_gives_the_same_result(dense, name):
    kw, laser = dense[name]
    for l in (None, laser):
        whole, wm = _run(kw, power=1, laser=l)
        parts, pm = _run(kw, power=1, laser=l, work_bytes=1)
        scale = float(wm.max())
        err = float((parts - whole).abs().max()) / scale
        print(f"{name} laser {l is not None}: one plane per chunk against unchunked: {err:.3e} of the maximum, "
              f"bitwise equal: {torch.equal(parts, whole) and torch.equal(pm, wm)}")
        assert err <= TOL_E2E


@pytest.mark.parametrize("name", ["12x20x48", "5x7x17_r3"])
def test_bitwise_repeatable_and_independent_of_the_row_order(dense, name):
    kw, laser = dense[name]
    H, W = kw["H"], kw["W"]
    rows = kw["rows"]
    for l in (None, laser):
        a, am = _run(kw, power=1, laser=l)
        b, bm = _run(kw, power=1, laser=l)
        assert torch.equal(a, b) and torch.equal(am, bm)
        order = np.random.default_rng(4).permutation(H * W)            # shuffled row u holds lattice point order[u]
        perm = _dev(np.argsort(order).astype(np.int32))
        assert torch.equal(a, _run(kw, rows=rows[order], power=1, laser=l, perm=perm)[0])
        t = np.arange(H * W).reshape(H, W).T.reshape(-1)               # the wall stored x-major
        assert torch.equal(a, _run(kw, rows=rows[t], power=1, laser=l, x_along="m")[0])


def test_errors(dense):
    kw, laser = dense["5x7x17_r3"]
    H, W = kw["H"], kw["W"]
    with pytest.raises(ValueError, match="depth"):
        _run(kw, ys=np.array([0.1, 0.3], dtype=np.float32))              # y0 = 0.1: a depth of zero
    with pytest.raises(ValueError, match="depth"):
        _run(kw, ys=np.array([0.05, 0.3], dtype=np.float32))
    with pytest.raises(ValueError, match="depth"):
        _run(kw, ys=np.array([0.3, float("nan")], dtype=np.float32))
    with pytest.raises(ValueError, match="Nt"):
        _run(kw, Nt=41)
    with pytest.raises(ValueError, match="Nt"):
        _run(kw, Nt=16)                                                  # shorter than the rows
    with pytest.raises(ValueError, match="power"):
        _run(kw, power=5)
    with pytest.raises(RuntimeError):
        _run(kw, perm=_dev(np.arange(H * W, dtype=np.int64)))
    with pytest.raises(ValueError):
        _run(kw, perm=_dev(np.full(H * W, H * W, dtype=np.int32)))
    with pytest.raises(ValueError):
        _run(kw, laser=(0.0, 0.1))
    with pytest.raises(ValueError):
        _run(kw, wavelength=0.1)                                         # P < 2 bins
    q_lo, _, nq = _band(kw)
    sx, sz = RO.spacings(kw["xs"], kw["zs"])
    strided = torch.empty((3, nq, 2 * H, 4 * W), dtype=torch.complex64, device=DEV)[..., ::2]
    with pytest.raises(ValueError, match="contiguous"):
        R.rsd_kernel(_dev(kw["ys"]), kw["y0"], H, W, sx, sz, kw["dr"], kw["Nt"], q_lo, nq, out=strided)
    with pytest.raises(RuntimeError, match="power"):                     # the library's own check, through the stage
        R.rsd_kernel(_dev(kw["ys"]), kw["y0"], H, W, sx, sz, kw["dr"], kw["Nt"], q_lo, nq, power=5)


@pytest.mark.parametrize("with_laser", [False, True], ids=["confocal", "one_laser"])
@pytest.mark.parametrize("name", list(FO.SCATTERERS))
def test_point_scatterer_peaks_at_its_voxel(name, with_laser):
    """The CPU-verified scenes (test_rsd_cpu): the fast field peaks at the scatterer's voxel, and so does
    phasor_backproject on the same voxels (VoxelGrid(tables=)).  The two magnitudes differ by definition (linear
    interpolation and truncated taps there, the band and the period here): the normalised difference is printed."""
    from nlosgr.phasor import phasor_backproject, phasor_kernel, phasor_rows
    from nlosgr.voxelize import VoxelGrid
    kw, laser, voxel = RO.scatterer_problem(name, with_laser)
    planes, mag = _run(kw, laser=laser)
    assert torch.isfinite(mag).all() and RO.argmax3(mag.cpu().numpy()) == voxel
    c = FO.SCATTERERS[name]
    _, _, walls = FO.lattice(c["H"], c["W"], c["sx"], c["sz"])
    grid = VoxelGrid(tables=tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in (kw["xs"], kw["ys"], kw["zs"])))
    rows_c = phasor_rows(_dev(kw["rows"]), phasor_kernel(kw["wavelength"], kw["dr"]))
    _, pmag = phasor_backproject(rows_c, _dev(walls), grid, kw["r0"], kw["dr"],
                                 lasers=None if laser is None else _dev(laser[None]))
    assert RO.argmax3(pmag.cpu().numpy()) == voxel
    diff = float((mag / mag.max() - pmag / pmag.max()).abs().max())
    print(f"{name} laser {with_laser}: |rsd / max - phasor_backproject / max| at most {diff:.3e}")


CAPTURE = "16x16x64_r20"
BOX = dict(position=(0.0, 0.7, 0.0), size=0.61)     # no lattice plane lies on a face of the box
RES = 9
WAVELENGTH = RO.SCATTERER_WAVELENGTH[CAPTURE] * FO.SCATTERERS[CAPTURE]["sx"]


def _write_capture(path, lasers=None):
    """The r0 = 20 dr scatterer as a capture file: 84 bins of a 16 x 16 wall, the window is bins [20, 84).  lasers:
    None (confocal), "one" (a [3, 1] field), "same" (that spot repeated), "each" (a distinct spot per point)."""
    from nlosgr.data import save_zaragoza
    c = FO.SCATTERERS[CAPTURE]
    kw, laser, voxel = RO.scatterer_problem(CAPTURE, lasers is not None)
    _, _, walls = FO.lattice(c["H"], c["W"], c["sx"], c["sz"])
    data = np.zeros((84, c["H"], c["W"]), dtype=np.float32)
    data[20:84] = kw["rows"].T.reshape(64, c["H"], c["W"])
    lg = None
    if lasers == "one":
        lg = laser.reshape(3, 1)
    elif lasers == "same":
        lg = np.repeat(laser.reshape(3, 1), c["H"] * c["W"], axis=1)
    elif lasers == "each":
        lg = (walls + np.array([0.1, 0.0, 0.0], dtype=np.float32)[None]).T
    save_zaragoza(str(path), data, walls.T, BOX["position"], BOX["size"], c["dr"], 1.0, laser_grid_positions=lg)
    return kw, laser


@pytest.mark.parametrize("lasers", [None, "one", "same"], ids=["confocal", "one_laser", "equal_spots"])
def test_rsd_capture_shuffled_unshuffled_and_cropped(tmp_path, lasers):
    from nlosgr.data import make_data_kwargs
    from nlosgr.voxelize import VoxelGrid
    c = FO.SCATTERERS[CAPTURE]
    kw, laser = _write_capture(tmp_path / "cap.mat", lasers)
    torch.manual_seed(6)
    dks, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=True)
    dku, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    assert not torch.equal(dks["index"], dku["index"])
    full = R.rsd_capture(dku, RES, 20, 84, WAVELENGTH, crop=False)
    assert sorted(full) == ["depth", "front", "grid", "imag", "real", "volume"]
    assert full["volume"].shape == full["real"].shape == full["imag"].shape == full["grid"].shape == (16, RES, 16)
    assert np.array_equal(full["grid"].xs.numpy(), kw["xs"]) and np.array_equal(full["grid"].zs.numpy(), kw["zs"])
    # the depths of phasor_capture: the y table of the capture's own box (its position is stored in fp32)
    want_ys = VoxelGrid([float(v) for v in dku["volume_position"]], float(dku["volume_size"]), RES).ys
    assert torch.equal(full["grid"].ys, want_ys)
    assert np.allclose(want_ys.numpy(), np.linspace(0.7 - 0.305, 0.7 + 0.305, RES), rtol=0, atol=1e-6)
    shuf = R.rsd_capture(dks, RES, 20, 84, WAVELENGTH, crop=False)
    for key in ("volume", "real", "imag"):
        assert torch.equal(full[key], shuf[key]), key
    # the volume is rsd_reconstruct's for the capture's rows, with its laser spot
    cdt = float(dku["c"]) * float(dku["deltaT"])
    planes, mag = R.rsd_reconstruct(_dev(kw["rows"]), 16, 16, kw["xs"], kw["zs"], 0.0, want_ys, 20 * cdt, cdt, WAVELENGTH,
                                    laser=laser)
    assert torch.equal(full["volume"], mag) and torch.equal(full["real"], planes[0]) and torch.equal(full["imag"], planes[1])
    assert torch.equal(full["front"], full["volume"].amax(dim=1))
    # the scatterer sits at depth 0.64; the nearest plane is index 3 (0.62375)
    n, _, m = c["voxel"]
    assert RO.argmax3(full["volume"].cpu().numpy()) == (n, 3, m)
    # crop: exactly the block of lattice points inside the volume box, every depth plane
    inside = []
    for t, p in ((full["grid"].xs, BOX["position"][0]), (full["grid"].zs, BOX["position"][2])):
        ok = np.nonzero((t.numpy() >= p - BOX["size"] / 2) & (t.numpy() <= p + BOX["size"] / 2))[0]
        inside.append((int(ok[0]), int(ok[-1]) + 1))
    (x0, x1), (z0, z1) = inside
    assert (x1 - x0, z1 - z0) == (10, 10)
    for dk in (dku, dks):
        crop = R.rsd_capture(dk, RES, 20, 84, WAVELENGTH)
        assert torch.equal(crop["volume"], full["volume"][x0:x1, :, z0:z1]) and crop["volume"].is_contiguous()
        assert torch.equal(crop["real"], full["real"][x0:x1, :, z0:z1]) and crop["real"].is_contiguous()
        assert crop["grid"].shape == (10, RES, 10) and torch.equal(crop["grid"].ys, want_ys)
        assert torch.equal(crop["grid"].xs, full["grid"].xs[x0:x1]) and torch.equal(crop["grid"].zs, full["grid"].zs[z0:z1])
        assert crop["front"].shape == crop["depth"].shape == (10, 10)


def test_rsd_capture_refuses_a_spot_per_point(tmp_path):
    from nlosgr.data import make_data_kwargs
    _write_capture(tmp_path / "nc.mat", "each")
    dk, *_ = make_data_kwargs(str(tmp_path / "nc.mat"), DEV, shuffle=False)
    with pytest.raises(NotImplementedError, match="nlosgr.phasor"):
        R.rsd_capture(dk, RES, 20, 84, WAVELENGTH)


def test_command_line_writes_the_npz(tmp_path):
    from nlosgr.data import make_data_kwargs
    from nlosgr.mesh import read_ply
    _write_capture(tmp_path / "cap.mat", "one")
    npz, ply = str(tmp_path / "rsd.npz"), str(tmp_path / "rsd.ply")
    R.main([str(tmp_path / "cap.mat"), "--resolution", str(RES), "--start", "20", "--end", "84", "--wavelength",
            str(WAVELENGTH), "--out", npz, "--mesh", ply])
    z = np.load(npz)
    assert sorted(z.files) == sorted(["density", "albedo", "front", "depth", "xs", "ys", "zs", "cam", "real", "imag"])
    dk, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    out = R.rsd_capture(dk, RES, 20, 84, WAVELENGTH)
    assert np.array_equal(z["density"], out["volume"].cpu().numpy()) and np.array_equal(z["albedo"], z["density"])
    assert np.array_equal(z["real"], out["real"].cpu().numpy()) and np.array_equal(z["imag"], out["imag"].cpu().numpy())
    assert np.array_equal(z["ys"], out["grid"].ys.numpy()) and read_ply(ply).vertices.shape[0] > 0


def test_initialiser_draws_from_the_rsd_volume(tmp_path):
    from nlosgr.data import make_data_kwargs
    from nlosgr.init import sample_from_backprojection
    c = FO.SCATTERERS[CAPTURE]
    kw, _ = _write_capture(tmp_path / "cap.mat", "one")
    dk, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    args = SimpleNamespace(init_gaussian_num=400, carving_volume_size=RES, start=20, end=84)
    np.random.seed(2)
    torch.manual_seed(2)
    pts, rho = sample_from_backprojection(args, dk, margin=0.1, method="rsd", wavelength=WAVELENGTH)
    assert pts.shape == (400, 3) and pts.is_cuda and rho.shape == (400, 1)
    pmin, pmax = dk["pmin"][:3], dk["pmax"][:3]
    lo, hi = pmin + (pmin * 0.1).abs(), pmax - (pmax * 0.1).abs()
    spacing = torch.tensor([c["sx"], BOX["size"] / (RES - 1), c["sz"]], device=DEV)    # the volume's own
    assert (pts >= lo - spacing / 2 - 1e-6).all() and (pts <= hi + spacing / 2 + 1e-6).all()
    n, j, m = c["voxel"]
    centre = torch.tensor([float(kw["xs"][n]), 20 * c["dr"] + j * c["dr"], float(kw["zs"][m])], device=DEV)
    near = (((pts - centre[None]).abs() <= 3 * spacing[None] + 1e-6).all(dim=1)).float().mean().item()
    print(f"share of the draws within three voxels of the scatterer {near:.3f}")
    assert near > 0.5
    with pytest.raises(ValueError, match="wavelength"):
        sample_from_backprojection(args, dk, margin=0.1, method="rsd")
    with pytest.raises(ValueError):
        sample_from_backprojection(args, dk, method="lct")
