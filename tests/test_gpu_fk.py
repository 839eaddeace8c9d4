"""GPU checks of f-k migration (include/nlosgr.h nlosgr_fk_load / _stolt / _store, csrc/nlosgr_fk.hip, nlosgr/fk.py)
against the float64 oracle of tests/fk_oracle.py, which starts from the fp32 inputs the kernels get.

Shapes are the smallest at which the kernels can go wrong: 16 x 16 x 64; 12 x 20 x 48 with sx != sz; 5 x 7 x 17 with
r0 = 3 dr (odd extents: a partial transpose tile on every axis, rows that are not 8-byte aligned, an odd pair at the
end of the band, the 4-byte store); 16 x 16 x 64 with r0 = 35 dr; 1 x 9 x 16, a single wall row.  The rows are dense
and seeded, non-negative but for a few negative entries, so every spectrum bin is exercised and the clamp is hit.

Tolerances.  End to end (per voxel, as a fraction of the volume's maximum) and the Stolt pass alone (per bin, as a
fraction of the largest |V|; the oracle is fed the GPU's own fp32 spectrum, so the FFT's error is not charged to the
kernel) are held to 4 x the worst value measured on the MI355X over all cases and options, one digit up (the rule of
DESIGN.md's parity tables), and may not exceed 2e-5 of the maximum, the cap the confocal forward is held to:

    end to end   measured 5.35e-7 (5 x 7 x 17, power 4, no amplitude)   4 x = 2.14e-6   tolerance 3e-6
    stolt        measured 4.86e-8 (5 x 7 x 17)                          4 x = 1.94e-7   tolerance 2e-7

The load pass is held per element to 8 x 2^-24 of the value: r = fma(j, dr, r0) carries 2^-24, r^4 = (r r)(r r)
four times that plus three roundings, the product with the bin one more: 8 x 2^-24 (the 1-ulp hardware square root
of the amplitude halves what came before it and adds 2^-23: 6 x 2^-24).  The store pass is within 2 fp32 ulp of
float32(re^2 + im^2).  Run with -s for the measured figures."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fk_oracle as FO
from nlosgr import fk as FK

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP = 2e-5            # of the maximum: no tolerance here may exceed it
TOL_E2E = 3e-6
TOL_STOLT = 2e-7
TOL_LOAD = 8 * 2.0 ** -24
OPTIONS = [(4, True), (0, True), (4, False), (0, False)]     # (power, amplitude)

assert TOL_E2E <= CAP and TOL_STOLT <= CAP


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def dense():
    """name -> (case, rows fp32, r0, dr), built once."""
    return {name: (c, FO.dense_rows(c), *FO.window(c)) for name, c in FO.DENSE.items()}


def _migrate(c, rows, r0, dr, **kw):
    return FK.fk_migrate(_dev(rows) if isinstance(rows, np.ndarray) else rows, c["H"], c["W"], c["sx"], c["sz"], r0, dr, **kw)


@pytest.mark.parametrize("name", list(FO.DENSE))
def test_end_to_end_against_the_oracle(dense, name):
    c, rows, r0, dr = dense[name]
    worst = 0.0
    for power, amp in OPTIONS:
        got = _migrate(c, rows, r0, dr, power=power, amplitude=amp)
        assert got.shape == (c["W"], c["nr"], c["H"]) and got.dtype == torch.float32 and got.is_contiguous()
        ref = FO.migrate64(rows, c["H"], c["W"], c["sx"], c["sz"], r0, dr, power=power, amplitude=amp)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max() / ref.max())
        print(f"{name} power {power} amplitude {amp}: end-to-end error {err:.3e} of the maximum (tolerance {TOL_E2E:g})")
        worst = max(worst, err)
    assert worst <= TOL_E2E, (name, worst)


@pytest.mark.parametrize("name", list(FO.DENSE))
def test_load_alone(dense, name):
    c, rows, r0, dr = dense[name]
    H, W, nr = c["H"], c["W"], c["nr"]
    assert (rows < 0).any()
    for power, amp in OPTIONS:
        out = torch.full((2 * H, 2 * W, 2 * nr), float("nan"), dtype=torch.complex64, device=DEV)
        got = FK.fk_load(_dev(rows), H, W, r0, dr, power=power, amplitude=amp, out=out)
        assert got.data_ptr() == out.data_ptr()
        g = got.cpu().numpy()
        ref = FO.load64(rows, H, W, r0, dr, power=power, amplitude=amp).real
        assert not np.isnan(g.view(np.float32)).any()
        assert not g.imag.any() and not g[H:].any() and not g[:, W:].any() and not g[:, :, nr:].any()
        assert (g.real[:H, :W, :nr][rows.reshape(H, W, nr) < 0] == 0).all()                 # the clamp
        rel = np.abs(g.real.astype(np.float64) - ref) / np.where(ref > 0, ref, 1.0)
        print(f"{name} power {power} amplitude {amp}: load worst relative error {rel.max() / 2.0 ** -24:.2f} x 2^-24")
        assert rel.max() <= TOL_LOAD, (name, power, amp)


@pytest.mark.parametrize("name", list(FO.DENSE))
def test_stolt_alone(dense, name):
    c, rows, r0, dr = dense[name]
    H, W, nr = c["H"], c["W"], c["nr"]
    spec = torch.fft.fftn(FK.fk_load(_dev(rows), H, W, r0, dr))
    out = torch.full_like(spec, float("nan"))
    got = FK.fk_stolt(spec, c["sx"], c["sz"], r0, dr, out=out)
    assert got.data_ptr() == out.data_ptr()
    g = got.cpu().numpy()
    ref = FO.stolt64(spec.cpu().numpy(), c["sx"], c["sz"], r0, dr)
    assert not np.isnan(g.view(np.float32)).any()
    zero = ref == 0
    assert zero[:, :, 0].all() and zero[:, :, max(nr - 1, 0):].all() and not g[zero].any()     # written, exactly zero
    if nr >= 3:
        assert (~zero).any()
        err = float(np.abs(g.astype(np.complex128) - ref).max() / np.abs(ref).max())
        print(f"{name}: stolt error {err:.3e} of the largest |V| (tolerance {TOL_STOLT:g})")
        assert err <= TOL_STOLT, (name, err)
    with pytest.raises(ValueError):
        FK.fk_stolt(spec, c["sx"], c["sz"], r0, dr, out=spec)
    # a work array that is not contiguous is refused, not silently copied
    strided = torch.empty((2 * H, 2 * W, 4 * nr), dtype=torch.complex64, device=DEV)[:, :, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        FK.fk_stolt(spec, c["sx"], c["sz"], r0, dr, out=strided)
    with pytest.raises(ValueError, match="contiguous"):
        FK.fk_load(_dev(rows), H, W, r0, dr, out=strided)


def _ulps(got, want):
    g, w = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert np.isfinite(g).all() and (g >= 0).all()
    return int(np.abs(g.view(np.int32).astype(np.int64) - w.view(np.int32).astype(np.int64)).max())


@pytest.mark.parametrize("name", list(FO.DENSE))
def test_store_alone(dense, name):
    c = dense[name][0]
    H, W, nr = c["H"], c["W"], c["nr"]
    g = np.random.default_rng(9)
    field = (g.standard_normal((2 * H, 2 * W, 2 * nr)) + 1j * g.standard_normal((2 * H, 2 * W, 2 * nr))).astype(np.complex64)
    field[H:] = field[:, W:] = field[:, :, nr:] = np.nan          # nothing outside the corner is read into the result
    got = FK.fk_store(_dev(field))
    assert got.shape == (W, nr, H)
    want = FO.store64(field, H, W, nr).astype(np.float32)
    u = _ulps(got.cpu().numpy(), want)
    print(f"{name}: store within {u} ulp of float32(re^2 + im^2)")
    assert u <= 2


@pytest.mark.parametrize("name", list(FO.SCATTERERS))
def test_point_scatterer_peaks_at_its_voxel(name):
    c = FO.SCATTERERS[name]
    rows, xs, zs, r0, dr = FO.scatterer_scene(c)
    vol = _migrate(c, rows, r0, dr)
    assert torch.isfinite(vol).all()
    at = tuple(int(v) for v in np.unravel_index(int(vol.argmax()), tuple(vol.shape)))
    assert at == c["voxel"]


@pytest.mark.parametrize("name", ["12x20x48", "5x7x17_r3"])
def test_bitwise_repeatable_and_independent_of_the_row_order(dense, name):
    c, rows, r0, dr = dense[name]
    H, W = c["H"], c["W"]
    a = _migrate(c, rows, r0, dr)
    assert torch.equal(a, _migrate(c, rows, r0, dr))
    order = np.random.default_rng(4).permutation(H * W)            # shuffled row u holds lattice point order[u]
    perm = _dev(np.argsort(order).astype(np.int32))
    assert torch.equal(a, _migrate(c, rows[order], r0, dr, perm=perm))
    t = np.arange(H * W).reshape(H, W).T.reshape(-1)               # the wall stored x-major
    assert torch.equal(a, _migrate(c, rows[t], r0, dr, x_along="m"))
    with pytest.raises(ValueError):
        _migrate(c, rows, r0, dr, perm=_dev(np.full(H * W, H * W, dtype=np.int32)))
    with pytest.raises(RuntimeError):
        _migrate(c, rows, r0, dr, perm=_dev(np.arange(H * W, dtype=np.int64)))
    with pytest.raises(RuntimeError, match="power"):
        _migrate(c, rows, r0, dr, power=5)


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


def test_fk_capture_shuffled_unshuffled_and_cropped(tmp_path):
    from nlosgr.data import make_data_kwargs
    c = CAPTURE
    rows, xs, zs = _write_capture(tmp_path / "cap.mat")
    torch.manual_seed(6)
    dks, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=True)
    dku, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    assert not torch.equal(dks["index"], dku["index"])
    full = FK.fk_capture(dku, 20, 84, crop=False)
    assert sorted(full) == ["depth", "front", "grid", "volume"]
    assert full["volume"].shape == full["grid"].shape == (16, 64, 16)
    assert np.array_equal(full["grid"].xs.numpy(), xs) and np.array_equal(full["grid"].zs.numpy(), zs)
    cdt = float(dku["c"]) * float(dku["deltaT"])
    assert np.array_equal(full["grid"].ys.numpy(), (0.0 + 20 * cdt + cdt * np.arange(64)).astype(np.float32))
    at = tuple(int(v) for v in np.unravel_index(int(full["volume"].argmax()), (16, 64, 16)))
    assert at == c["voxel"]
    assert torch.equal(full["volume"], FK.fk_capture(dks, 20, 84, crop=False)["volume"])
    # the volume is fk_migrate's for the capture's rows
    want = FK.fk_migrate(_dev(rows), 16, 16, FK.lattice_spacing(full["grid"].xs), FK.lattice_spacing(full["grid"].zs),
                         20 * cdt, cdt)
    assert torch.equal(full["volume"], want)
    assert torch.equal(full["front"], full["volume"].amax(dim=1))
    # crop: exactly the block of the voxels inside the volume box
    inside = []
    for t, p in zip(full["grid"].tables, BOX["position"]):
        ok = np.nonzero((t.numpy() >= p - BOX["size"] / 2) & (t.numpy() <= p + BOX["size"] / 2))[0]
        inside.append((int(ok[0]), int(ok[-1]) + 1))
    (x0, x1), (y0, y1), (z0, z1) = inside
    assert (x1 - x0, y1 - y0, z1 - z0) == (10, 31, 10)
    for dk in (dku, dks):
        crop = FK.fk_capture(dk, 20, 84)
        assert torch.equal(crop["volume"], full["volume"][x0:x1, y0:y1, z0:z1]) and crop["volume"].is_contiguous()
        assert crop["grid"].shape == (10, 31, 10) and torch.equal(crop["grid"].ys, full["grid"].ys[y0:y1])
        assert torch.equal(crop["grid"].xs, full["grid"].xs[x0:x1]) and torch.equal(crop["grid"].zs, full["grid"].zs[z0:z1])
        assert crop["front"].shape == crop["depth"].shape == (10, 10)


def test_fk_capture_refuses_a_non_confocal_capture(tmp_path):
    from nlosgr.data import make_data_kwargs
    _write_capture(tmp_path / "nc.mat", lasers=True)
    dk, *_ = make_data_kwargs(str(tmp_path / "nc.mat"), DEV, shuffle=False)
    with pytest.raises(NotImplementedError, match="nlosgr.phasor"):
        FK.fk_capture(dk, 20, 84)


def test_command_line_writes_the_npz(tmp_path):
    from nlosgr.data import make_data_kwargs
    from nlosgr.mesh import read_ply
    _write_capture(tmp_path / "cap.mat")
    npz, ply = str(tmp_path / "fk.npz"), str(tmp_path / "fk.ply")
    FK.main([str(tmp_path / "cap.mat"), "--start", "20", "--end", "84", "--out", npz, "--mesh", ply])
    z = np.load(npz)
    assert sorted(z.files) == sorted(["density", "albedo", "front", "depth", "xs", "ys", "zs", "cam"])
    dk, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    out = FK.fk_capture(dk, 20, 84)
    assert np.array_equal(z["density"], out["volume"].cpu().numpy()) and np.array_equal(z["albedo"], z["density"])
    assert np.array_equal(z["ys"], out["grid"].ys.numpy()) and read_ply(ply).vertices.shape[0] > 0


def test_initialiser_draws_from_the_fk_volume(tmp_path):
    from nlosgr.backproject import backproject_capture
    from nlosgr.data import make_data_kwargs
    from nlosgr.init import sample_from_backprojection
    c = CAPTURE
    _, xs, zs = _write_capture(tmp_path / "cap.mat")
    dk, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    args = SimpleNamespace(init_gaussian_num=400, carving_volume_size=9, start=20, end=84)
    np.random.seed(2)
    torch.manual_seed(2)
    pts, rho = sample_from_backprojection(args, dk, margin=0.1, method="fk")
    assert pts.shape == (400, 3) and pts.is_cuda and rho.shape == (400, 1)
    pmin, pmax = dk["pmin"][:3], dk["pmax"][:3]
    lo, hi = pmin + (pmin * 0.1).abs(), pmax - (pmax * 0.1).abs()
    spacing = torch.tensor([c["sx"], c["dr"], c["sz"]], device=DEV)       # the f-k grid's own, not the carving cube's
    assert (pts >= lo - spacing / 2 - 1e-6).all() and (pts <= hi + spacing / 2 + 1e-6).all()
    n, j, m = c["voxel"]
    centre = torch.tensor([float(xs[n]), 20 * c["dr"] + j * c["dr"], float(zs[m])], device=DEV)
    near = (((pts - centre[None]).abs() <= 3 * spacing[None] + 1e-6).all(dim=1)).float().mean().item()
    print(f"share of the draws within three voxels of the scatterer {near:.3f}")
    assert near > 0.5
    # the default method is the back-projection sampler as it was: the same calls on the same generators
    np.random.seed(3)
    torch.manual_seed(3)
    got, grho = sample_from_backprojection(args, dk, margin=0.1)
    np.random.seed(3)
    torch.manual_seed(3)
    wrho = np.random.rand(400, 1) * 0.1
    out = backproject_capture(dk, 9, 20, 84, power=0, filter="log", positive=True)
    vol, grid = out["volume"], out["grid"]
    gx, gy, gz = grid.on(DEV)
    inside = (((gx >= lo[0]) & (gx <= hi[0]))[:, None, None] & ((gy >= lo[1]) & (gy <= hi[1]))[None, :, None]
              & ((gz >= lo[2]) & (gz <= hi[2]))[None, None, :])
    w = torch.where(inside, vol, torch.zeros_like(vol)).reshape(-1).double()
    idx = torch.multinomial(w / w.sum(), 400, replacement=True)
    base = torch.stack((gx[idx // 81], gy[(idx // 9) % 9], gz[idx % 9]), dim=1)
    half = ((pmax - pmin) / 8) / 2.0
    want = base + (torch.rand_like(base) - 0.5) * 2 * half[None]
    assert torch.equal(got, want) and np.array_equal(grho, wrho)
    np.random.seed(3)
    torch.manual_seed(3)
    again, _ = sample_from_backprojection(args, dk, margin=0.1, method="backprojection", power=0)
    assert torch.equal(got, again)
    # `power` belongs to the back-projection: the f-k volume's weight is fk_power, 4 unless given
    import inspect
    sig = inspect.signature(sample_from_backprojection).parameters
    assert sig["power"].default == 0 and sig["fk_power"].default == 4 and sig["method"].default == "backprojection"
    np.random.seed(2)
    torch.manual_seed(2)
    same, _ = sample_from_backprojection(args, dk, margin=0.1, method="fk", power=2, fk_power=4)
    assert torch.equal(same, pts)
    with pytest.raises(ValueError):
        sample_from_backprojection(args, dk, method="lct")
