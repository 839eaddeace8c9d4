"""GPU checks of the primal-dual LCT solver (nlosgr.lct.lct_solve_pd, lct_solve_capture's new arguments, the command
line's; nlosgr.prox.primal_dual) against the float64 loop of tests/prox_oracle.py over lct_op_oracle.Operator64.

Thirty iterations on the five point-scatterer scenes of lct_op_oracle.peak_solution, with tv = 0.01 lambda0,
l1 = 0.05 lambda0 and axis weights (1, 0.5, 1.5); the steps come from the float64 norm (times NORM_SAFETY).
  mse       the scene's rows times r^3, tau = sigma = 1 / sqrt(L).
  poisson   the scene's raw rows with gt_times bringing their maximum to 200 counts, rate_floor 1 and the exposure
            r^-3 (0 at r = 0); sigma = 30 / sqrt(L), tau = 1 / (30 sqrt(L)): with equal steps the dual of a count
            likelihood needs hundreds of iterations to leave zero, and thirty would test nothing.
objective and terms follow the float64 loop's, relative per iteration (a term that is 0 in float64 must be 0), within
4 x the worst value measured on the MI355X, one digit up, and never above 2e-5, the cap of test_gpu_lct.py:

    objective and terms   measured 2.80e-6 (12x20x48, poisson, the TV and L1 terms)   4 x = 1.12e-5   tolerance 2e-5

The objectives alone stay within 3.6e-7 and the data terms within 3.9e-7; the TV and L1 terms, sums over the small
entries of a sparse iterate, within 1.2e-6 (mse) and 2.8e-6 (poisson).  The phantom gives Phi 19082 against 29055
and TV 866 against 1686 on the MI355X.

Run with -s for the measured figures."""
import functools

import numpy as np
import pytest
import torch

import fk_oracle as FO
import lct_oracle as LO
import lct_op_oracle as OO
import prox_oracle as PO
from nlosgr import lct as LCT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP = 2e-5
TOL_PD = 2e-5
WEIGHTS = (1.0, 0.5, 1.5)
TV_FRACTION, L1_FRACTION = 0.01, 0.05

assert TOL_PD <= CAP


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _exposure(r0, dr, nr, falloff=3.0):
    r = FO.f32(r0) + np.arange(nr) * FO.f32(dr)
    return np.where(r > 0, np.where(r > 0, r, 1.0) ** -falloff, 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _solution(index, loss):
    """The float64 loop of one scene, computed once: the inputs as fp32, the steps, and (volume, objective, terms)."""
    s = OO.peak_solution(index)
    c = s["case"]
    op = OO.Operator64(c["H"], c["W"], c["sx"], c["sz"], s["r0"], s["dr"], c["nr"], 0, s["nv"])
    norm = LCT.NORM_SAFETY * s["norm"]
    root = np.sqrt(norm + 4.0 * sum(w * w for w in WEIGHTS))
    if loss == "mse":
        h, e, gt, k = s["rows"], None, 1.0, 1.0
    else:
        h = FO.scatterer_scene(c)[0]
        e, gt, k = _exposure(s["r0"], s["dr"], c["nr"]), float(np.float32(200.0 / h.max())), 30.0
    lam = PO.lambda0(op, h, loss, e, gt, 1.0)
    kw = dict(tv=TV_FRACTION * lam, l1=L1_FRACTION * lam, loss=loss, sigma=k / root, tau=1.0 / (k * root))
    out = PO.primal_dual(op, h, 30, norm, e=e, gt=gt, eps=1.0, a=WEIGHTS, **kw)
    return dict(s=s, h=h, e=e, gt=gt, norm=norm, lam=lam, kw=kw, out=out)


@pytest.mark.parametrize("loss", ["mse", "poisson"])
@pytest.mark.parametrize("index", range(len(LO.PEAKS)))
def test_thirty_iterations_follow_the_float64_loop(index, loss):
    f = _solution(index, loss)
    s, c = f["s"], f["s"]["case"]
    x64, obj64, terms64 = f["out"]
    at64 = tuple(int(v) for v in np.unravel_index(int(x64.argmax()), x64.shape))
    assert at64 == c["voxel"] and (x64 >= 0).all() and obj64[-1] < obj64[0]       # the oracle's own sanity
    op = LCT.LctOperator(c["H"], c["W"], c["sx"], c["sz"], s["r0"], s["dr"], c["nr"], power=0, nv=s["nv"], device=DEV)
    kw = dict(iterations=30, exposure=None if f["e"] is None else _dev(f["e"]), gt_times=f["gt"], rate_floor=1.0,
              weights=WEIGHTS, norm=f["norm"], **f["kw"])
    vol, obj, terms = LCT.lct_solve_pd(_dev(f["h"]), op, **kw)
    assert vol.shape == op.volume_shape and vol.dtype == torch.float32
    assert obj.shape == (30,) and terms.shape == (30, 3) and obj.dtype == terms.dtype == torch.float64 and obj.is_cuda
    o, t = obj.cpu().numpy(), terms.cpu().numpy()
    assert (t[terms64 == 0] == 0).all()
    rel_o = np.abs(o - obj64) / obj64
    rel_t = np.abs(t - terms64) / np.where(terms64 > 0, terms64, 1.0)
    name = f"{LO.PEAKS[index][0]} nv {s['nv']} {loss}"
    print(f"{name}: objective {o[0]:.6g} -> {o[-1]:.6g}; worst relative gap to float64: objective {rel_o.max():.3e}, "
          f"F {rel_t[:, 0].max():.3e}, TV {rel_t[:, 1].max():.3e}, L1 {rel_t[:, 2].max():.3e} (tolerance {TOL_PD:g})")
    assert rel_o.max() <= TOL_PD and rel_t.max() <= TOL_PD
    assert np.allclose(o, t @ np.array([1.0, f["kw"]["tv"], f["kw"]["l1"]]), rtol=1e-14, atol=0.0)
    at = tuple(int(v) for v in np.unravel_index(int(vol.argmax()), tuple(vol.shape)))
    assert at == c["voxel"] and float(vol.min()) >= 0.0
    vol2, obj2, terms2 = LCT.lct_solve_pd(_dev(f["h"]), op, **kw)
    assert torch.equal(vol, vol2) and torch.equal(obj, obj2) and torch.equal(terms, terms2)


def test_default_steps_and_arguments():
    f = _solution(2, "mse")
    s, c = f["s"], f["s"]["case"]
    op = LCT.LctOperator(c["H"], c["W"], c["sx"], c["sz"], s["r0"], s["dr"], c["nr"], device=DEV)
    rows = _dev(f["h"])
    # the default norm is NORM_SAFETY op.norm(): the same two objectives to the norm's own accuracy
    _, obj, _ = LCT.lct_solve_pd(rows, op, iterations=2, tv=f["kw"]["tv"], l1=f["kw"]["l1"], weights=WEIGHTS)
    assert abs(float(obj[1]) / f["out"][1][1] - 1.0) <= 1e-4
    # tv = l1 = 0 without the clamp from x0: one step of the plain iteration
    x0 = _dev(np.random.default_rng(3).standard_normal(op.volume_shape).astype(np.float32))
    vol, obj, terms = LCT.lct_solve_pd(rows, op, iterations=1, nonneg=False, x0=x0, norm=f["norm"])
    step = 1.0 / np.sqrt(f["norm"])
    z = op.forward(x0)
    want = x0 - step * op.adjoint((step * (z - rows)) / (1.0 + step))
    assert float((vol - want).abs().max()) <= 1e-5 * float(want.abs().max()) and float(vol.min()) < 0
    assert abs(float(terms[0, 2]) / float(x0.double().abs().sum()) - 1.0) <= 1e-12 and float(obj[0]) == float(terms[0, 0])
    with pytest.raises(ValueError):
        LCT.lct_solve_pd(rows[:-1].contiguous(), op)
    with pytest.raises(ValueError):
        LCT.lct_solve_pd(rows, op, x0=x0[:-1].contiguous())
    with pytest.raises(ValueError, match="exposure"):
        LCT.lct_solve_pd(rows, op, exposure=torch.ones(c["nr"], device=DEV))
    with pytest.raises(ValueError, match="iterations"):
        LCT.lct_solve_pd(rows, op, iterations=0)


def test_tv_beats_least_squares_on_a_noisy_phantom():
    """Two boxes (1 and 0.5) on the 16 x 16 x 64 lattice that starts at bin 20, rendered with op.forward, scaled to
    a peak of 5 counts and drawn from a seeded Poisson generator.  Sixty iterations each of lct_solve_pd at
    tv = 0.3 lambda0 and of lct_solve; Phi = 1/2 |A x - h|^2 + tv TV(x) is evaluated by the float64 oracle.  The
    float64 loops alone give Phi 19317 against 29465 and TV 881 against 1711."""
    c = FO.SCATTERERS["16x16x64_r20"]
    r0, dr = FO.window(c)
    op = LCT.LctOperator(c["H"], c["W"], c["sx"], c["sz"], r0, dr, c["nr"], device=DEV)
    truth = np.zeros(op.volume_shape, dtype=np.float32)
    truth[4:10, 20:32, 5:12] = 1.0
    truth[10:14, 40:50, 2:6] = 0.5
    clean = np.maximum(op.forward(_dev(truth)).cpu().numpy().astype(np.float64), 0.0)
    counts = np.random.default_rng(21).poisson(clean * (5.0 / clean.max())).astype(np.float32)
    rows = _dev(counts)
    lam = float(op.adjoint(rows).max())
    tv = 0.3 * lam
    x_pd, _, _ = LCT.lct_solve_pd(rows, op, iterations=60, tv=tv)
    x_ls, _ = LCT.lct_solve(rows, op, iterations=60)
    ref = OO.Operator64(c["H"], c["W"], c["sx"], c["sz"], r0, dr, c["nr"], 0)
    pd = PO.functional(ref, x_pd.cpu().numpy(), counts, tv)
    ls = PO.functional(ref, x_ls.cpu().numpy(), counts, tv)
    print(f"phantom: Phi {pd[0]:.6g} (primal-dual) against {ls[0]:.6g} (least squares); TV {pd[2]:.6g} against "
          f"{ls[2]:.6g}; data term {pd[1]:.6g} against {ls[1]:.6g}")
    assert pd[0] < 0.8 * ls[0] and pd[2] < 0.7 * ls[2]
    assert float(x_pd.min()) >= 0.0


CAPTURE = FO.SCATTERERS["16x16x64_r20"]
BOX = dict(position=(0.0, 0.7, 0.0), size=0.61)


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
    return rows


def test_lct_solve_capture(tmp_path):
    from nlosgr.data import make_data_kwargs
    c = CAPTURE
    rows = _write_capture(tmp_path / "cap.mat")
    torch.manual_seed(6)
    dks, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=True)
    dku, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    assert not torch.equal(dks["index"], dku["index"])
    cdt = float(dku["c"]) * float(dku["deltaT"])
    radii = 20 * cdt + cdt * torch.arange(64, dtype=torch.float64, device=DEV)
    op = LCT.LctOperator(16, 16, c["sx"], c["sz"], 20 * cdt, cdt, 64, device=DEV)
    scaled = (_dev(rows).double() * radii.pow(3.0)[None]).float()
    # the defaults: lct_solve's volume and today's keys
    plain = LCT.lct_solve_capture(dku, 20, 84, iterations=8, crop=False)
    assert sorted(plain) == ["depth", "front", "grid", "objective", "volume"]
    want, wobj = LCT.lct_solve(scaled, op, iterations=8, accelerate=True)
    assert torch.equal(plain["volume"], want) and torch.equal(plain["objective"], wobj)
    # tv and l1 are fractions of lambda0 = max A^T h
    lam = float(op.adjoint(scaled).max())
    out = LCT.lct_solve_capture(dku, 20, 84, iterations=10, crop=False, tv=0.02, l1=0.05, weights=WEIGHTS)
    assert sorted(out) == ["depth", "front", "grid", "lambda0", "objective", "terms", "volume"]
    assert out["lambda0"] == lam and out["terms"].shape == (10, 3) and out["objective"].shape == (10,)
    vol, obj, terms = LCT.lct_solve_pd(scaled, op, iterations=10, tv=0.02 * lam, l1=0.05 * lam, weights=WEIGHTS)
    assert torch.equal(out["volume"], vol) and torch.equal(out["objective"], obj) and torch.equal(out["terms"], terms)
    assert not torch.equal(vol, want) and float(vol.max()) > 0
    shuffled = LCT.lct_solve_capture(dks, 20, 84, iterations=10, crop=False, tv=0.02, l1=0.05, weights=WEIGHTS)
    assert torch.equal(shuffled["volume"], vol) and shuffled["lambda0"] == lam
    cropped = LCT.lct_solve_capture(dks, 20, 84, iterations=10, tv=0.02, l1=0.05, weights=WEIGHTS)
    assert cropped["volume"].shape == (10, 31, 10) and cropped["terms"].shape == (10, 3)
    # loss="poisson": raw counts, the falloff as the exposure table, the operator at power 0
    gt = float(np.float32(200.0 / rows.max()))
    e = torch.where(radii > 0, radii.pow(-3.0), torch.zeros_like(radii)).float()
    pull = (_dev(rows).double().mul(gt).clamp(min=0) * (e.double() / 1.0)[None]).float()
    lam_p = float(op.adjoint(pull).max())
    for dk in (dku, dks):
        out = LCT.lct_solve_capture(dk, 20, 84, iterations=10, crop=False, tv=0.01, l1=0.02, loss="poisson", gt_times=gt)
        assert out["lambda0"] == lam_p
        vol, obj, terms = LCT.lct_solve_pd(_dev(rows), op, iterations=10, tv=0.01 * lam_p, l1=0.02 * lam_p,
                                           loss="poisson", exposure=e, gt_times=gt, rate_floor=1.0)
        assert torch.equal(out["volume"], vol)
        assert torch.allclose(out["terms"], terms, rtol=1e-12, atol=0.0)          # (the rows' own order in the sums)
    assert torch.equal(out["terms"][:, 1:], terms[:, 1:])
    # above lambda0 the zero volume is the minimiser: exactly zero after 20 iterations, for both losses
    for kw in (dict(), dict(loss="poisson", gt_times=gt)):
        out = LCT.lct_solve_capture(dku, 20, 84, iterations=20, crop=False, l1=1.001, **kw)
        assert not out["volume"].any() and float(out["terms"][-1, 2]) == 0.0, kw
    assert LCT.lct_solve_capture(dku, 20, 84, iterations=20, crop=False, l1=0.05)["volume"].any()
    _write_capture(tmp_path / "nc.mat", lasers=True)
    dk, *_ = make_data_kwargs(str(tmp_path / "nc.mat"), DEV, shuffle=False)
    with pytest.raises(NotImplementedError, match="nlosgr.phasor"):
        LCT.lct_solve_capture(dk, 20, 84, tv=0.1)


def test_command_line(tmp_path):
    from nlosgr.data import make_data_kwargs
    _write_capture(tmp_path / "cap.mat")
    cap = str(tmp_path / "cap.mat")
    plain, solved, counted = (str(tmp_path / n) for n in ("plain.npz", "solved.npz", "counted.npz"))
    base = [cap, "--start", "20", "--end", "84", "--nv", "96", "--iterations", "6"]
    dk, *_ = make_data_kwargs(cap, DEV, shuffle=False)
    keys = sorted(["density", "albedo", "front", "depth", "xs", "ys", "zs", "cam", "objective"])
    # without the new flags: today's file, key for key and value for value
    LCT.main(base + ["--out", plain])
    z = np.load(plain)
    want = LCT.lct_solve_capture(dk, 20, 84, iterations=6, nv=96)
    assert sorted(z.files) == keys
    assert z["density"].tobytes() == want["volume"].cpu().numpy().tobytes()
    assert z["objective"].tobytes() == want["objective"].cpu().numpy().tobytes()
    assert z["front"].tobytes() == want["front"].cpu().numpy().tobytes()
    assert z["depth"].tobytes() == want["depth"].cpu().numpy().tobytes()
    assert np.array_equal(z["ys"], want["grid"].ys.numpy()) and np.array_equal(z["albedo"], z["density"])
    # with --tv: terms and lambda0 too, the density the function call's
    LCT.main(base + ["--tv", "0.02", "--l1", "0.05", "--out", solved])
    z = np.load(solved)
    want = LCT.lct_solve_capture(dk, 20, 84, iterations=6, nv=96, tv=0.02, l1=0.05)
    assert sorted(z.files) == sorted(keys + ["terms", "lambda0"])
    assert np.array_equal(z["density"], want["volume"].cpu().numpy()) and z["terms"].shape == (6, 3)
    assert np.array_equal(z["terms"], want["terms"].cpu().numpy()) and float(z["lambda0"]) == want["lambda0"]
    assert np.array_equal(z["objective"], want["objective"].cpu().numpy())
    LCT.main(base + ["--loss", "poisson", "--gt-times", "50", "--rate-floor", "0.5", "--l1", "0.01", "--out", counted])
    z = np.load(counted)
    want = LCT.lct_solve_capture(dk, 20, 84, iterations=6, nv=96, l1=0.01, loss="poisson", gt_times=50.0, rate_floor=0.5)
    assert np.array_equal(z["density"], want["volume"].cpu().numpy()) and float(z["lambda0"]) == want["lambda0"]
