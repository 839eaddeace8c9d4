"""GPU checks of the light-cone transform (include/nlosgr.h nlosgr_lct_load / _kernel / _filter / _store,
csrc/nlosgr_lct.hip, nlosgr/lct.py) against the float64 oracle of tests/lct_oracle.py, which starts from the fp32
inputs the kernels get.

Shapes are the dense cases of tests/fk_oracle.py, the smallest at which the kernels can go wrong: 16 x 16 x 64;
12 x 20 x 48 with sx != sz; 5 x 7 x 17 with r0 = 3 dr (odd extents: partial tiles on every axis, rows that are not
8-byte aligned, an odd cell at the end of a column) at nv = nr, 2 nr and 23; 16 x 16 x 64 with r0 = 35 dr; 1 x 9 x 16,
a single wall row; and two lattices of this file for the paths those do not reach, 2 x 3 x 40 at nv = 300 (more than
256 cells in a column, a store tile whose cells come in five chunks) and 3 x 2 x 300 at nv = 130 (more than 256 bins
in a row, five store tiles along time, runs of 20 bins).  The rows are dense and seeded, non-negative but for a few negative entries (the clamp is hit).

Measured tolerances.  End to end (per voxel, as a fraction of the volume's maximum) and the filter pass alone (the
product per element as a fraction of the largest |spec G|, the inverse alone as a fraction of the largest |G|; the
oracle is fed the GPU's own fp32 spectra, so the FFT's error is not charged to the kernel) are held to 4 x the worst
value measured on the MI355X over all cases and options, one digit up (the rule of DESIGN.md's parity tables), and may
not exceed 2e-5 of the maximum, the cap of test_gpu_fk.py:

    end to end   measured 1.75e-6 (2 x 3 x 40, nv 300, power 0, snr 100)      4 x = 7.01e-6   tolerance 8e-6
    filter       measured 1.48e-7 (12 x 20 x 48, the inverse at snr 100;
                 the product 1.23e-7, 16 x 16 x 64 r0 = 35 dr, snr 100)       4 x = 5.94e-7   tolerance 6e-7

End to end, the worst per snr and route over the nine cases: snr 0.8 3.90e-7, snr 100 1.75e-6, back-projection
4.12e-7; a sharp filter amplifies the FFTs' rounding.

Derived tolerances (u = 2^-24, the relative error of one fp32 rounding).
  load    Every term is non-negative, so the bound is relative per element.  psi carries 8 u (test_gpu_fk.py: r, r^4
          and the product with the bin), the fp32 weight 1 u, and acc = fma(w, psi, acc) rounds once per term of a
          run of at most L terms, each rounding relative to a partial sum that is at most the result:
          (1 + u)^(9 + L) - 1, with L the longest run of the case's operator.
  kernel  scale (1 - f) and scale f are formed in fp64 by the oracle's own operations (no contraction) and rounded
          to fp32 once: u of the value, plus 2^-149 for a value in the denormal range.
  store   |got - want| <= ((1 + u)^(1 + L) - 1) sum_i R[i, j] |Re o[m, n, i]|: 1 u for the weight, one rounding per
          term of a run of at most L cells, relative to at most the sum of the magnitudes; max(., 0) does not
          stretch a difference.
Run with -s for the measured figures."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fk_oracle as FO
import lct_oracle as LO
from nlosgr import lct as LCT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
CAP = 2e-5            # of the maximum: no measured tolerance here may exceed it
TOL_E2E = 8e-6
TOL_FILTER = 6e-7
OPTIONS = [(4, 0.8, False), (0, 0.8, False), (4, 100.0, False), (0, 100.0, False), (4, 0.8, True), (0, 0.8, True)]
# two more lattices for the paths the five above do not reach: more than 256 cells in a column (a lane's second pair)
# and a store tile whose cells come in five chunks; more than 256 bins in a row and five store tiles along time
EXTRA = {
    "2x3x40_r5": dict(H=2, W=3, nr=40, sx=0.1, sz=0.12, dr=0.02, r0_bins=5),
    "3x2x300_r10": dict(H=3, W=2, nr=300, sx=0.1, sz=0.1, dr=0.004, r0_bins=10),
}
CASES = ([(name, None) for name in FO.DENSE] + [("5x7x17_r3", 34), ("5x7x17_r3", 23)]
         + [("2x3x40_r5", 300), ("3x2x300_r10", 130)])
IDS = [f"{name}-nv{'=nr' if nv is None else nv}" for name, nv in CASES]

assert TOL_E2E <= CAP and TOL_FILTER <= CAP


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def dense():
    """name -> (case, rows fp32, r0, dr), built once."""
    return {name: (c, FO.dense_rows(c), *FO.window(c)) for name, c in {**FO.DENSE, **EXTRA}.items()}


def _reconstruct(c, rows, r0, dr, **kw):
    return LCT.lct_reconstruct(_dev(rows) if isinstance(rows, np.ndarray) else rows, c["H"], c["W"], c["sx"], c["sz"],
                               r0, dr, **kw)


def _longest(start):
    return int(np.diff(start.numpy()).max())


@pytest.mark.parametrize("name,nv", CASES, ids=IDS)
def test_end_to_end_against_the_oracle(dense, name, nv):
    c, rows, r0, dr = dense[name]
    worst = 0.0
    for power, snr, backprop in OPTIONS:
        got = _reconstruct(c, rows, r0, dr, power=power, snr=snr, nv=nv, backprop=backprop)
        assert got.shape == (c["W"], c["nr"], c["H"]) and got.dtype == torch.float32 and got.is_contiguous()
        ref = LO.reconstruct64(rows, c["H"], c["W"], c["sx"], c["sz"], r0, dr, power=power, snr=snr, nv=nv,
                               backprop=backprop)
        assert ref.max() > 0
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max() / ref.max())
        print(f"{name} nv {nv} power {power} snr {snr:g} backprop {backprop}: end-to-end error {err:.3e} of the "
              f"maximum (tolerance {TOL_E2E:g})")
        worst = max(worst, err)
    assert worst <= TOL_E2E, (name, nv, worst)


@pytest.mark.parametrize("name,nv", CASES, ids=IDS)
def test_load_alone(dense, name, nv):
    c, rows, r0, dr = dense[name]
    H, W, nr = c["H"], c["W"], c["nr"]
    assert (rows < 0).any()
    res = LCT.lct_resampling(r0, dr, nr, nv)
    R64, _ = LO.resampling64(r0, dr, nr, nv)
    tol = (1.0 + U) ** (9 + _longest(res.start)) - 1.0
    zero_rows = np.where(rows > 0, -rows, rows)                     # nothing positive: the result is exactly zero
    for power in (4, 0, 1, 2, 3):
        out = torch.full((2 * H, 2 * W, 2 * res.nv), float("nan"), dtype=torch.complex64, device=DEV)
        got = LCT.lct_load(_dev(rows), H, W, r0, dr, power=power, nv=nv, out=out)
        assert got.data_ptr() == out.data_ptr()
        g = got.cpu().numpy()
        ref = LO.load64(rows, H, W, r0, dr, R64, power=power).real
        assert not np.isnan(g.view(np.float32)).any()
        assert not g.imag.any() and not g[H:].any() and not g[:, W:].any() and not g[:, :, res.nv:].any()
        assert not g.real[ref == 0].any() and (ref[:H, :W, :res.nv] > 0).mean() > 0.9
        rel = np.abs(g.real.astype(np.float64) - ref) / np.where(ref > 0, ref, 1.0)
        print(f"{name} nv {nv} power {power}: load worst relative error {rel.max() / U:.2f} u (bound {tol / U:.2f} u)")
        assert rel.max() <= tol, (name, nv, power)
        assert not LCT.lct_load(_dev(zero_rows), H, W, r0, dr, power=power, resampling=res).cpu().numpy().any()


@pytest.mark.parametrize("name,nv", CASES, ids=IDS)
def test_kernel_alone(dense, name, nv):
    c, rows, r0, dr = dense[name]
    H, W = c["H"], c["W"]
    res = LCT.lct_resampling(r0, dr, c["nr"], nv)
    out = torch.full((2 * H, 2 * W, 2 * res.nv), float("nan"), dtype=torch.complex64, device=DEV)
    got = LCT.lct_kernel(H, W, res.nv, c["sx"], c["sz"], res.dv, out=out)
    assert got.data_ptr() == out.data_ptr()
    g = got.cpu().numpy()
    scale = LCT.lct_scale(H, W, res.nv, c["sx"], c["sz"], res.dv)       # what the kernel was given
    assert abs(scale / LO.kernel64(H, W, res.nv, c["sx"], c["sz"], res.dv)[1] - 1.0) <= 1e-14
    ref, _ = LO.kernel64(H, W, res.nv, c["sx"], c["sz"], res.dv, scale=scale)
    assert not np.isnan(g.view(np.float32)).any() and not g.imag.any()
    assert np.array_equal(g.real != 0, ref != 0) and (ref != 0).any()
    diff = np.abs(g.real.astype(np.float64) - ref)
    assert (diff <= U * ref + 2.0 ** -149).all(), (name, nv, float((diff / np.where(ref > 0, ref, 1.0)).max() / U))
    print(f"{name} nv {nv}: kernel worst relative error {float((diff / np.where(ref > 0, ref, 1.0)).max() / U):.2f} u, "
          f"{int((ref != 0).sum())} non-zeros, norm {float(np.sqrt((g.real.astype(np.float64) ** 2).sum())):.9f}")


@pytest.mark.parametrize("name,nv", CASES, ids=IDS)
def test_filter_alone(dense, name, nv):
    c, rows, r0, dr = dense[name]
    H, W = c["H"], c["W"]
    res = LCT.lct_resampling(r0, dr, c["nr"], nv)
    spec = torch.fft.fftn(LCT.lct_load(_dev(rows), H, W, r0, dr, resampling=res))
    kf = torch.fft.fftn(LCT.lct_kernel(H, W, res.nv, c["sx"], c["sz"], res.dv))
    s64, k64 = spec.cpu().numpy(), kf.cpu().numpy()
    worst = 0.0
    for snr, backprop in ((0.8, False), (100.0, False), (0.8, True)):
        out = torch.full_like(spec, float("nan"))
        got = LCT.lct_filter(spec, kf=kf, snr=snr, backprop=backprop, out=out)
        assert got.data_ptr() == out.data_ptr()
        g = got.cpu().numpy()
        assert not np.isnan(g.view(np.float32)).any()
        G64 = LO.inverse64(k64, snr, backprop)
        ref = s64.astype(np.complex128) * G64
        err = float(np.abs(g.astype(np.complex128) - ref).max() / np.abs(ref).max())
        print(f"{name} nv {nv} snr {snr:g} backprop {backprop}: filter error {err:.3e} of the largest |spec G| "
              f"(tolerance {TOL_FILTER:g})")
        worst = max(worst, err)
        # the inverse alone, and the product with a stored inverse: the same bits as the fused pass
        G = LCT.lct_filter(None, kf=kf, snr=snr, backprop=backprop)
        gerr = float(np.abs(G.cpu().numpy().astype(np.complex128) - G64).max() / np.abs(G64).max())
        print(f"{name} nv {nv} snr {snr:g} backprop {backprop}: inverse error {gerr:.3e} of the largest |G|")
        worst = max(worst, gerr)
        assert torch.equal(torch.view_as_real(LCT.lct_filter(spec, inverse=G)), torch.view_as_real(got))
        inplace = spec.clone()
        assert LCT.lct_filter(inplace, inverse=G, out=inplace).data_ptr() == inplace.data_ptr()
        assert torch.equal(torch.view_as_real(inplace), torch.view_as_real(got))
    assert worst <= TOL_FILTER, (name, nv, worst)
    strided = torch.empty((2 * H, 2 * W, 4 * res.nv), dtype=torch.complex64, device=DEV)[:, :, ::2]
    for call in (lambda: LCT.lct_filter(spec, kf=kf, out=strided),
                 lambda: LCT.lct_kernel(H, W, res.nv, c["sx"], c["sz"], res.dv, out=strided),
                 lambda: LCT.lct_load(_dev(rows), H, W, r0, dr, resampling=res, out=strided)):
        with pytest.raises(ValueError, match="contiguous"):
            call()
    with pytest.raises(ValueError):
        LCT.lct_filter(spec, kf=kf[:, :, :-2].contiguous())


@pytest.mark.parametrize("name,nv", CASES, ids=IDS)
def test_store_alone(dense, name, nv):
    c, rows, r0, dr = dense[name]
    H, W, nr = c["H"], c["W"], c["nr"]
    res = LCT.lct_resampling(r0, dr, nr, nv)
    R64, _ = LO.resampling64(r0, dr, nr, nv)
    shape = (2 * H, 2 * W, 2 * res.nv)
    g = np.random.default_rng(9)
    field = (g.standard_normal(shape) + 1j * g.standard_normal(shape)).astype(np.complex64)
    field[H:] = field[:, W:] = field[:, :, res.nv:] = np.nan      # nothing outside the corner is read into the result
    got = LCT.lct_store(_dev(field), res)
    assert got.shape == (W, nr, H) and got.dtype == torch.float32 and got.is_contiguous()
    got = got.cpu().numpy().astype(np.float64)
    want, scale = LO.store64(field, H, W, R64), LO.store_scale64(field, H, W, R64)
    tol = (1.0 + U) ** (1 + _longest(res.start_t)) - 1.0
    assert np.isfinite(got).all() and (got >= 0).all() and (got == 0).any() and (got > 0).any()
    rel = np.abs(got - want) / scale
    print(f"{name} nv {nv}: store worst error {rel.max() / U:.2f} u of sum R |Re o| (bound {tol / U:.2f} u)")
    assert rel.max() <= tol, (name, nv)
    with pytest.raises(ValueError):
        LCT.lct_store(_dev(field), LCT.lct_resampling(r0, dr, nr, res.nv + 1))


@pytest.mark.parametrize("name,nv,voxel", LO.PEAKS)
def test_point_scatterer_peaks_at_its_voxel(name, nv, voxel):
    c = LO.peak_case(name, voxel)
    rows, xs, zs, r0, dr = FO.scatterer_scene(c)
    for snr in (0.8, 100.0):
        vol = _reconstruct(c, rows, r0, dr, snr=snr, nv=nv)
        assert torch.isfinite(vol).all()
        at = tuple(int(v) for v in np.unravel_index(int(vol.argmax()), tuple(vol.shape)))
        assert at == c["voxel"], (snr, at)


@pytest.mark.parametrize("name,nv", [("12x20x48", None), ("5x7x17_r3", 23)])
def test_bitwise_repeatable_and_independent_of_the_row_order(dense, name, nv):
    c, rows, r0, dr = dense[name]
    H, W = c["H"], c["W"]
    a = _reconstruct(c, rows, r0, dr, nv=nv)
    assert torch.equal(a, _reconstruct(c, rows, r0, dr, nv=nv))
    order = np.random.default_rng(4).permutation(H * W)            # shuffled row u holds lattice point order[u]
    perm = _dev(np.argsort(order).astype(np.int32))
    assert torch.equal(a, _reconstruct(c, rows[order], r0, dr, nv=nv, perm=perm))
    t = np.arange(H * W).reshape(H, W).T.reshape(-1)               # the wall stored x-major
    assert torch.equal(a, _reconstruct(c, rows[t], r0, dr, nv=nv, x_along="m"))
    # an inverse built once and passed in: the same bits, for the Wiener filter and for the adjoint
    res = LCT.lct_resampling(r0, dr, c["nr"], nv)
    G = LCT.lct_inverse(H, W, res.nv, c["sx"], c["sz"], res.dv, 0.8)
    assert G.shape == (2 * H, 2 * W, 2 * res.nv) and G.dtype == torch.complex64
    keep = G.clone()
    assert torch.equal(a, _reconstruct(c, rows, r0, dr, nv=nv, inverse=G))
    assert torch.equal(torch.view_as_real(G), torch.view_as_real(keep))                       # left as it was
    Gb = LCT.lct_inverse(H, W, res.nv, c["sx"], c["sz"], res.dv, 0.8, backprop=True)
    b = _reconstruct(c, rows, r0, dr, nv=nv, backprop=True)
    assert torch.equal(b, _reconstruct(c, rows, r0, dr, nv=nv, inverse=Gb)) and not torch.equal(a, b)
    with pytest.raises(ValueError):
        _reconstruct(c, rows, r0, dr, nv=nv, perm=_dev(np.full(H * W, H * W, dtype=np.int32)))
    with pytest.raises(RuntimeError):
        _reconstruct(c, rows, r0, dr, nv=nv, perm=_dev(np.arange(H * W, dtype=np.int64)))
    with pytest.raises(RuntimeError, match="power"):
        _reconstruct(c, rows, r0, dr, nv=nv, power=5)
    for snr in (0.0, -2.0):
        with pytest.raises(ValueError, match="snr"):
            _reconstruct(c, rows, r0, dr, nv=nv, snr=snr)
    with pytest.raises(ValueError, match="nv"):
        _reconstruct(c, rows, r0, dr, nv=0)
    with pytest.raises(ValueError):
        _reconstruct(c, rows, r0, dr, nv=nv, inverse=G[:, :, :-2].contiguous())


CAPTURE = FO.SCATTERERS["16x16x64_r20"]
BOX = dict(position=(0.0, 0.7, 0.0), size=0.61)     # no lattice plane lies on a face of the box


def _write_capture(path, lasers=False):
    """The r0 = 20 dr scatterer as a capture file: 84 bins of a 16 x 16 wall, the window is bins [20, 84)."""
    from nlosgr.data import save_zaragoza
    c = CAPTURE
    rows, xs, zs, r0, dr = FO.scatterer_scene(c)
    _, _, walls = FO.lattice(c["H"], c["W"], c["sx"], c["sz"])
    data = np.zeros((84, c["H"], c["W"]), dtype=np.float32)
    data[20:84] = rows.T.reshape(64, c["H"], c["W"])
    lg = (walls + np.array([0.1, 0.0, 0.0], dtype=np.float32)[None]).T if lasers else None
    save_zaragoza(str(path), data, walls.T, BOX["position"], BOX["size"], c["dr"], 1.0, laser_grid_positions=lg)
    return rows, xs, zs


def test_lct_capture_shuffled_unshuffled_and_cropped(tmp_path):
    from nlosgr.data import make_data_kwargs
    from nlosgr.fk import lattice_spacing
    c = CAPTURE
    rows, xs, zs = _write_capture(tmp_path / "cap.mat")
    torch.manual_seed(6)
    dks, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=True)
    dku, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    assert not torch.equal(dks["index"], dku["index"])
    full = LCT.lct_capture(dku, 20, 84, crop=False)
    assert sorted(full) == ["depth", "front", "grid", "volume"]
    assert full["volume"].shape == full["grid"].shape == (16, 64, 16)
    assert np.array_equal(full["grid"].xs.numpy(), xs) and np.array_equal(full["grid"].zs.numpy(), zs)
    cdt = float(dku["c"]) * float(dku["deltaT"])
    assert np.array_equal(full["grid"].ys.numpy(), (0.0 + 20 * cdt + cdt * np.arange(64)).astype(np.float32))
    at = tuple(int(v) for v in np.unravel_index(int(full["volume"].argmax()), (16, 64, 16)))
    assert at == c["voxel"]
    assert torch.equal(full["volume"], LCT.lct_capture(dks, 20, 84, crop=False)["volume"])
    # the volume is lct_reconstruct's for the capture's rows; the options reach it
    sx, sz = lattice_spacing(full["grid"].xs), lattice_spacing(full["grid"].zs)
    want = LCT.lct_reconstruct(_dev(rows), 16, 16, sx, sz, 20 * cdt, cdt)
    assert torch.equal(full["volume"], want)
    want = LCT.lct_reconstruct(_dev(rows), 16, 16, sx, sz, 20 * cdt, cdt, power=2, snr=10.0, nv=100)
    assert torch.equal(LCT.lct_capture(dks, 20, 84, power=2, snr=10.0, nv=100, crop=False)["volume"], want)
    assert torch.equal(full["front"], full["volume"].amax(dim=1))
    # crop: exactly the block of the voxels inside the volume box
    inside = []
    for t, p in zip(full["grid"].tables, BOX["position"]):
        ok = np.nonzero((t.numpy() >= p - BOX["size"] / 2) & (t.numpy() <= p + BOX["size"] / 2))[0]
        inside.append((int(ok[0]), int(ok[-1]) + 1))
    (x0, x1), (y0, y1), (z0, z1) = inside
    assert (x1 - x0, y1 - y0, z1 - z0) == (10, 31, 10)
    for dk in (dku, dks):
        crop = LCT.lct_capture(dk, 20, 84)
        assert torch.equal(crop["volume"], full["volume"][x0:x1, y0:y1, z0:z1]) and crop["volume"].is_contiguous()
        assert crop["grid"].shape == (10, 31, 10) and torch.equal(crop["grid"].ys, full["grid"].ys[y0:y1])
        assert torch.equal(crop["grid"].xs, full["grid"].xs[x0:x1]) and torch.equal(crop["grid"].zs, full["grid"].zs[z0:z1])
        assert crop["front"].shape == crop["depth"].shape == (10, 10)


def test_lct_capture_refuses_a_non_confocal_capture_and_a_wall_that_is_no_lattice(tmp_path):
    from nlosgr.data import make_data_kwargs
    _write_capture(tmp_path / "nc.mat", lasers=True)
    dk, *_ = make_data_kwargs(str(tmp_path / "nc.mat"), DEV, shuffle=False)
    with pytest.raises(NotImplementedError, match="nlosgr.phasor"):
        LCT.lct_capture(dk, 20, 84)
    _write_capture(tmp_path / "cap.mat")
    dk, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    bent = dict(dk)
    pos = dk["camera_grid_positions"].clone()
    pos[0] = pos[0] * pos[0].abs()                                 # non-uniform spacing
    bent["camera_grid_positions"] = pos
    with pytest.raises(ValueError, match="lattice"):
        LCT.lct_capture(bent, 20, 84)


def test_command_line_writes_the_npz(tmp_path):
    from nlosgr.data import make_data_kwargs
    from nlosgr.mesh import read_ply
    _write_capture(tmp_path / "cap.mat")
    npz, ply = str(tmp_path / "lct.npz"), str(tmp_path / "lct.ply")
    LCT.main([str(tmp_path / "cap.mat"), "--start", "20", "--end", "84", "--snr", "2", "--nv", "96", "--out", npz,
              "--mesh", ply])
    z = np.load(npz)
    assert sorted(z.files) == sorted(["density", "albedo", "front", "depth", "xs", "ys", "zs", "cam"])
    dk, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    out = LCT.lct_capture(dk, 20, 84, snr=2.0, nv=96)
    assert np.array_equal(z["density"], out["volume"].cpu().numpy()) and np.array_equal(z["albedo"], z["density"])
    assert np.array_equal(z["ys"], out["grid"].ys.numpy()) and read_ply(ply).vertices.shape[0] > 0


def test_initialiser_draws_from_the_lct_volume(tmp_path):
    from nlosgr.data import make_data_kwargs
    from nlosgr.init import sample_from_volume
    c = CAPTURE
    _, xs, zs = _write_capture(tmp_path / "cap.mat")
    dk, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    out = LCT.lct_capture(dk, 20, 84)
    args = SimpleNamespace(init_gaussian_num=400)
    np.random.seed(2)
    torch.manual_seed(2)
    pts, rho = sample_from_volume(args, dk, **{k: out[k] for k in ("volume", "grid")})
    assert pts.shape == (400, 3) and pts.is_cuda and rho.shape == (400, 1) and (rho >= 0).all() and (rho <= 0.1).all()
    pmin, pmax = dk["pmin"][:3], dk["pmax"][:3]
    lo, hi = pmin + (pmin * 0.1).abs(), pmax - (pmax * 0.1).abs()
    spacing = torch.tensor([c["sx"], c["dr"], c["sz"]], device=DEV)       # the volume's own grid
    assert (pts >= lo - spacing / 2 - 1e-6).all() and (pts <= hi + spacing / 2 + 1e-6).all()
    n, j, m = c["voxel"]
    centre = torch.tensor([float(xs[n]), 20 * c["dr"] + j * c["dr"], float(zs[m])], device=DEV)
    near = (((pts - centre[None]).abs() <= 3 * spacing[None] + 1e-6).all(dim=1)).float().mean().item()
    print(f"share of the draws within three voxels of the scatterer {near:.3f}")
    assert near > 0.5
    np.random.seed(2)
    torch.manual_seed(2)
    again, _ = sample_from_volume(args, dk, out["volume"], out["grid"])
    assert torch.equal(pts, again)
    with pytest.raises(RuntimeError, match="nothing to sample"):
        sample_from_volume(args, dk, torch.zeros_like(out["volume"]), out["grid"])
