"""GPU checks of the LCT operator pair (include/nlosgr.h nlosgr_lct_load_volume / _store_rows / _load_rows /
_store_volume, csrc/nlosgr_lct.hip, nlosgr.lct.LctOperator, lct_solve, lct_solve_capture, VoxelFitStep(operator=))
against the float64 oracle of tests/lct_op_oracle.py, which starts from the fp32 inputs the kernels get.

Shapes.  The five dense lattices of tests/fk_oracle.py at nv = nr (1 x 9 x 16 keeps H = 1); 5 x 7 x 17 at nv 34 and 23;
2 x 3 x 40 at nv 300 (more than 256 cells in a column, five cell tiles in load_volume); 3 x 2 x 300 at nv 130 (more
than 256 bins, several 64-bin chunks and tiles); and 70 x 2 x 20, the only one with H > 64: two z tiles, the second
partial, in the two transposing passes.  Inputs are signed and seeded.

Derived tolerances (u = 2^-24, L the longest run of the case's tables; the oracle is given the operator's own fp32
weights, Resampling.dense(), so their rounding is not in the budget).  Per element, relative to the sum of the
absolute terms:
  load_volume, store_volume   (1 + u)^(1 + L) - 1: one rounding per fmaf term.
  load_rows, store_rows       (1 + u)^(L + |power| + 4) - 1: the fmaf for r, the multiplications, the division, the
                              product with the bin, one rounding per fmaf term.

Measured tolerances.  End to end (forward against project64, adjoint against adjoint64, signed input, per element as
a fraction of the output's maximum) and the adjoint identity on the device (|<A v, h> - <v, A^T h>| with float64 dot
products over ||A v|| ||h||) are held to 4 x the worst value measured on the MI355X over all cases and powers, one digit
up, and may not exceed 2e-5, the cap of test_gpu_lct.py:

    end to end         measured 4.46e-7 (5 x 7 x 17, nv 23, forward, power 4)    4 x = 1.78e-6   tolerance 2e-6
    adjoint identity   measured 2.19e-8 (5 x 7 x 17, nv 23, power -3)            4 x = 8.74e-8   tolerance 9e-8

All 120 end-to-end figures lie in 8.39e-8 ... 4.46e-7, the 60 gaps in 1.71e-11 ... 2.19e-8.  The stage checks reach at
most 2.02 u (load_volume, store_volume; bounds 3 - 21 u) and 6.43 u (load_rows, store_rows; bounds 6 - 28 u).  Thirty
Landweber objectives stay within 8.0e-8 (relative) of the float64 solver's.

Run with -s for the measured figures."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fk_oracle as FO
import lct_oracle as LO
import lct_op_oracle as OO
from nlosgr import lct as LCT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
CAP = 2e-5
TOL_E2E = 2e-6
TOL_ADJOINT = 9e-8
POWERS = (-4, -3, -1, 0, 2, 4)
EXTRA = {
    "2x3x40_r5": dict(H=2, W=3, nr=40, sx=0.1, sz=0.12, dr=0.02, r0_bins=5),
    "3x2x300_r10": dict(H=3, W=2, nr=300, sx=0.1, sz=0.1, dr=0.004, r0_bins=10),
    "70x2x20": dict(H=70, W=2, nr=20, sx=0.1, sz=0.1, dr=0.03, r0_bins=3),
}
LATTICES = {**FO.DENSE, **EXTRA}
CASES = ([(name, None) for name in FO.DENSE] + [("5x7x17_r3", 34), ("5x7x17_r3", 23)]
         + [("2x3x40_r5", 300), ("3x2x300_r10", 130), ("70x2x20", None)])
IDS = [f"{name}-nv{'=nr' if nv is None else nv}" for name, nv in CASES]

assert TOL_E2E <= CAP and TOL_ADJOINT <= CAP


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _longest(start):
    return int(np.diff(start.numpy()).max())


def _inputs(name):
    """(case, r0, dr, signed volume [W, nr, H] fp32, signed rows [H W, nr] fp32), seeded by the lattice."""
    c = LATTICES[name]
    g = np.random.default_rng(100 + c["H"] * 1000 + c["W"] * 10 + c["nr"])
    vol = g.standard_normal((c["W"], c["nr"], c["H"])).astype(np.float32)
    rows = g.standard_normal((c["H"] * c["W"], c["nr"])).astype(np.float32)
    return (c, *FO.window(c), vol, rows)


def _field(H, W, nv, seed=9):
    """A random complex64 field [2H, 2W, 2nv], NaN outside the [0:H, 0:W, 0:nv] corner."""
    g = np.random.default_rng(seed)
    shape = (2 * H, 2 * W, 2 * nv)
    field = (g.standard_normal(shape) + 1j * g.standard_normal(shape)).astype(np.complex64)
    field[H:] = field[:, W:] = field[:, :, nv:] = np.nan
    return field


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _padding_is_zero(g, H, W, nv):
    assert not np.isnan(g.view(np.float32)).any()
    assert not g.imag.any() and not g[H:].any() and not g[:, W:].any() and not g[:, :, nv:].any()


def _operator(c, r0, dr, **kw):
    return LCT.LctOperator(c["H"], c["W"], c["sx"], c["sz"], r0, dr, c["nr"], device=DEV, **kw)


def _oracle(c, r0, dr, **kw):
    return OO.Operator64(c["H"], c["W"], c["sx"], c["sz"], r0, dr, c["nr"], **kw)


@pytest.mark.parametrize("name,nv", CASES, ids=IDS)
def test_load_volume_and_store_volume_alone(name, nv):
    c, r0, dr, vol, _ = _inputs(name)
    H, W, nr = c["H"], c["W"], c["nr"]
    res = LCT.lct_resampling(r0, dr, nr, nv)
    R = res.dense().numpy()
    out = _nan((2 * H, 2 * W, 2 * res.nv), torch.complex64)
    got = LCT.lct_load_volume(_dev(vol), res, out=out)
    assert got.data_ptr() == out.data_ptr()
    g = got.cpu().numpy()
    _padding_is_zero(g, H, W, res.nv)
    v64 = vol.astype(np.float64).transpose(2, 0, 1)
    want, scale = v64 @ R.T, np.abs(v64) @ R.T
    tol = (1.0 + U) ** (1 + _longest(res.start)) - 1.0
    rel = np.abs(g.real[:H, :W, :res.nv].astype(np.float64) - want) / scale
    print(f"{name} nv {nv}: load_volume worst error {rel.max() / U:.2f} u of sum R |v| (bound {tol / U:.2f} u)")
    assert rel.max() <= tol and (want < 0).any(), (name, nv)
    assert torch.equal(torch.view_as_real(LCT.lct_load_volume(_dev(vol), res)), torch.view_as_real(got))

    field = _field(H, W, res.nv)
    got = LCT.lct_store_volume(_dev(field), res)
    assert got.shape == (W, nr, H) and got.dtype == torch.float32 and got.is_contiguous()
    got = got.cpu().numpy().astype(np.float64)
    o = field[:H, :W, :res.nv].real.astype(np.float64)
    want, scale = (o @ R).transpose(1, 2, 0), (np.abs(o) @ R).transpose(1, 2, 0)
    tol = (1.0 + U) ** (1 + _longest(res.start_t)) - 1.0
    assert np.isfinite(got).all() and (got < 0).any() and (got > 0).any()
    rel = np.abs(got - want) / scale
    print(f"{name} nv {nv}: store_volume worst error {rel.max() / U:.2f} u of sum R |Re o| (bound {tol / U:.2f} u)")
    assert rel.max() <= tol, (name, nv)
    # where the sum is >= 0 these are the bits of the clamped store
    clamped = LCT.lct_store(_dev(field), res).cpu().numpy()
    assert np.array_equal(np.maximum(got, 0.0), clamped.astype(np.float64))


@pytest.mark.parametrize("name,nv", CASES, ids=IDS)
def test_load_rows_and_store_rows_alone(name, nv):
    c, r0, dr, _, rows = _inputs(name)
    H, W, nr = c["H"], c["W"], c["nr"]
    res = LCT.lct_resampling(r0, dr, nr, nv)
    R = res.dense().numpy()
    field = _field(H, W, res.nv)
    o = field[:H, :W, :res.nv].real.astype(np.float64)
    h64 = rows.astype(np.float64).reshape(H, W, nr)
    L, Lt = _longest(res.start), _longest(res.start_t)
    for power in POWERS:
        w = OO.weights64(r0, dr, nr, power)
        assert np.isfinite(w).all() and (w[1:] > 0).all()
        if r0 == 0.0 and power < 0:
            assert w[0] == 0.0                                        # not inf: the kernels must give 0 there too
        out = _nan((2 * H, 2 * W, 2 * res.nv), torch.complex64)
        got = LCT.lct_load_rows(_dev(rows), H, W, r0, dr, power=power, nv=nv, out=out)
        assert got.data_ptr() == out.data_ptr()
        g = got.cpu().numpy()
        _padding_is_zero(g, H, W, res.nv)
        want, scale = (h64 * w) @ R.T, (np.abs(h64) * w) @ R.T
        tol = (1.0 + U) ** (L + abs(power) + 4) - 1.0
        rel = np.abs(g.real[:H, :W, :res.nv].astype(np.float64) - want) / np.where(scale > 0, scale, 1.0)
        print(f"{name} nv {nv} power {power}: load_rows worst error {rel.max() / U:.2f} u (bound {tol / U:.2f} u)")
        assert rel.max() <= tol, (name, nv, power)

        out = _nan((H * W, nr), torch.float32)
        got = LCT.lct_store_rows(_dev(field), res, power=power, out=out)
        assert got.data_ptr() == out.data_ptr()
        g = got.cpu().numpy().astype(np.float64).reshape(H, W, nr)
        assert np.isfinite(g).all()
        want, scale = (o @ R) * w, (np.abs(o) @ R) * w
        tol = (1.0 + U) ** (Lt + abs(power) + 4) - 1.0
        rel = np.abs(g - want) / np.where(scale > 0, scale, 1.0)
        print(f"{name} nv {nv} power {power}: store_rows worst error {rel.max() / U:.2f} u (bound {tol / U:.2f} u)")
        assert rel.max() <= tol and (want < 0).any(), (name, nv, power)
    # bitwise link: on non-negative rows and powers 0..4, load_rows gives the bits of lct_load
    for power in range(5):
        a = LCT.lct_load_rows(_dev(np.abs(rows)), H, W, r0, dr, power=power, resampling=res)
        b = LCT.lct_load(_dev(np.abs(rows)), H, W, r0, dr, power=power, resampling=res)
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)), (name, nv, power)
    for power in (-5, 5):
        with pytest.raises(ValueError, match="power"):
            LCT.lct_load_rows(_dev(rows), H, W, r0, dr, power=power, resampling=res)
        with pytest.raises(ValueError, match="power"):
            LCT.lct_store_rows(_dev(field), res, power=power)
    with pytest.raises(ValueError):
        LCT.lct_store_rows(_dev(field), res, perm=_dev(np.full(H * W, H * W, dtype=np.int32)))


def test_store_rows_leaves_the_rows_no_lattice_point_names():
    c, r0, dr, _, _ = _inputs("5x7x17_r3")
    H, W, nr = c["H"], c["W"], c["nr"]
    res = LCT.lct_resampling(r0, dr, nr)
    field = _dev(_field(H, W, res.nv))
    plain = LCT.lct_store_rows(field, res, power=-3)
    perm = np.arange(H * W, dtype=np.int32)
    perm[0] = perm[1] = 3                                             # rows 0 and 1 are named by no point
    keep = np.float32(7.5)
    out = torch.full((H * W, nr), float(keep), device=DEV)
    got = LCT.lct_store_rows(field, res, power=-3, perm=_dev(perm), out=out)
    assert (got[:2] == keep).all() and torch.equal(got[4:], plain[4:]) and torch.equal(got[2], plain[2])


@pytest.mark.parametrize("name,nv", CASES, ids=IDS)
def test_forward_and_adjoint_against_the_oracle(name, nv):
    c, r0, dr, vol, rows = _inputs(name)
    worst = gap_worst = 0.0
    for power in POWERS:
        op, ref = _operator(c, r0, dr, power=power, nv=nv), _oracle(c, r0, dr, power=power, nv=nv)
        assert op.Fk.shape == (2 * c["H"], 2 * c["W"], 2 * op.nv) and op.Fk.dtype == torch.complex64
        Av, Ath = op.forward(_dev(vol)), op.adjoint(_dev(rows))
        assert Av.shape == op.rows_shape == rows.shape and Ath.shape == op.volume_shape == vol.shape
        assert Av.dtype == Ath.dtype == torch.float32 and Av.is_contiguous() and Ath.is_contiguous()
        for what, got, want in (("forward", Av, ref.forward(vol)), ("adjoint", Ath, ref.adjoint(rows))):
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
            print(f"{name} nv {nv} power {power}: {what} error {err:.3e} of the maximum (tolerance {TOL_E2E:g})")
            worst = max(worst, err)
        lhs = float((Av.double() * _dev(rows).double()).sum())
        rhs = float((_dev(vol).double() * Ath.double()).sum())
        gap = abs(lhs - rhs) / (float(Av.double().norm()) * float(np.sqrt((rows.astype(np.float64) ** 2).sum())))
        print(f"{name} nv {nv} power {power}: adjoint identity gap {gap:.3e} (tolerance {TOL_ADJOINT:g})")
        gap_worst = max(gap_worst, gap)
        # a second run gives the same bits; the one-call forms are the operator's
        assert torch.equal(Av, op.forward(_dev(vol))) and torch.equal(Ath, op.adjoint(_dev(rows)))
    assert torch.equal(Av, LCT.lct_project(_dev(vol), c["H"], c["W"], c["sx"], c["sz"], r0, dr, power=power, nv=nv))
    assert torch.equal(Ath, LCT.lct_adjoint(_dev(rows), c["H"], c["W"], c["sx"], c["sz"], r0, dr, power=power, nv=nv))
    assert worst <= TOL_E2E, (name, nv, worst)
    assert gap_worst <= TOL_ADJOINT, (name, nv, gap_worst)


@pytest.mark.parametrize("name,nv", CASES, ids=IDS)
def test_adjoint_has_the_bits_of_the_transforms_back_projection(name, nv):
    """On non-negative rows and powers 0..4 the adjoint is lct_reconstruct(backprop=True) wherever that is not
    clamped (the FFTs leave a few sums a rounding below zero)."""
    c, r0, dr, _, rows = _inputs(name)
    rows = _dev(np.abs(rows))
    for power in range(5):
        got = _operator(c, r0, dr, power=power, nv=nv).adjoint(rows)
        want = LCT.lct_reconstruct(rows, c["H"], c["W"], c["sx"], c["sz"], r0, dr, power=power, nv=nv, backprop=True)
        assert torch.equal(got.clamp_min(0.0), want), (name, nv, power)
        assert float(got.min()) >= -1e-5 * float(got.max())


@pytest.mark.parametrize("name,nv", [("12x20x48", None), ("5x7x17_r3", 23), ("70x2x20", None)])
def test_independent_of_the_row_order(name, nv):
    c, r0, dr, vol, rows = _inputs(name)
    H, W = c["H"], c["W"]
    vol, rows = _dev(vol), _dev(rows)
    plain = _operator(c, r0, dr, power=-3, nv=nv)
    Av, Ath = plain.forward(vol), plain.adjoint(rows)
    order = np.random.default_rng(4).permutation(H * W)              # shuffled row u holds lattice point order[u]
    shuffled = _operator(c, r0, dr, power=-3, nv=nv, perm=_dev(np.argsort(order).astype(np.int32)))
    assert torch.equal(shuffled.forward(vol), Av[_dev(order)])
    assert torch.equal(shuffled.adjoint(rows[_dev(order)].contiguous()), Ath)
    t = np.arange(H * W).reshape(H, W).T.reshape(-1)                 # the wall stored x-major
    xmajor = _operator(c, r0, dr, power=-3, nv=nv, x_along="m")
    assert torch.equal(xmajor.forward(vol), Av[_dev(t)])
    assert torch.equal(xmajor.adjoint(rows[_dev(t)].contiguous()), Ath)
    with pytest.raises(ValueError):
        _operator(c, r0, dr, perm=_dev(np.full(H * W, H * W, dtype=np.int32)))
    with pytest.raises(ValueError):
        plain.forward(vol[:, :-1].contiguous())
    with pytest.raises(ValueError):
        plain.adjoint(rows[:-1].contiguous())


def test_power_minus_three_is_the_physical_confocal_transient():
    """A Gaussian blob of std 0.08 at voxel (10, 22, 5) of the r0 = 20 dr lattice: scale_to_physical * A at power
    -3 against forward_project at power -4 on the operator's grid.  The two discretisations differ by 2.3e-2
    (rel-L2; the LCT's cell model is not a hat splat), and fp32 gives the float64 oracles' figure to 1e-3."""
    import forward_project_oracle as PO
    from nlosgr.forward_project import forward_project
    c = FO.SCATTERERS["16x16x64_r20"]
    H, W, nr = c["H"], c["W"], c["nr"]
    xs, zs, walls = FO.lattice(H, W, c["sx"], c["sz"])
    r0, dr = FO.window(c)
    vol = OO.blob(c, (10, 22, 5), 0.08, xs, zs, r0, dr)
    op = _operator(c, r0, dr, power=-3)
    grid = op.grid(xs, zs, 0.0)
    assert grid.shape == op.volume_shape
    mine = op.scale_to_physical * LCT.lct_project(_dev(vol), H, W, c["sx"], c["sz"], r0, dr, power=-3).double()
    exact = forward_project(_dev(vol), _dev(walls), grid, r0, dr, nr, power=-4).double()
    got = float((mine - exact).norm() / exact.norm())
    ref = _oracle(c, r0, dr, power=-3)
    scale64 = ref.dv / (2.0 * dr * ref.scale)
    assert abs(op.scale_to_physical / scale64 - 1.0) <= 1e-12
    ys = grid.ys.numpy()
    inv_dr = float(np.float32(1.0) / np.float32(dr))
    exact64, _ = PO.forward64(vol, walls, xs, ys, zs, r0, inv_dr, nr, -4, want_bound=False)
    mine64 = scale64 * ref.forward(vol)
    want = float(np.sqrt(((mine64 - exact64) ** 2).sum() / (exact64 ** 2).sum()))
    print(f"physical match: rel-L2 {got:.5f} on the GPU, {want:.5f} in float64, scale {scale64:.4f}")
    assert 0.01 < want < 0.04 and abs(got - want) <= 1e-3


@pytest.mark.parametrize("index", range(len(LO.PEAKS)))
def test_solvers_on_a_point_scatterer(index):
    s = OO.peak_solution(index)
    c, rows = s["case"], _dev(s["rows"])
    op = _operator(c, s["r0"], s["dr"], power=0, nv=s["nv"])
    norm = op.norm()
    print(f"{LO.PEAKS[index][0]} nv {s['nv']}: norm {norm:.8g}, float64 {s['norm']:.8g}")
    assert abs(norm / s["norm"] - 1.0) <= 1e-5
    step = 1.0 / s["norm"]
    vol, obj = LCT.lct_solve(rows, op, iterations=30, step=step)
    assert vol.shape == op.volume_shape and obj.shape == (30,) and obj.dtype == torch.float64 and obj.is_cuda
    obj = obj.cpu().numpy()
    rel = np.abs(obj - s["landweber"][1]) / s["landweber"][1]
    print(f"  Landweber objective {obj[0]:.6g} -> {obj[-1]:.6g}, worst relative gap to float64 {rel.max():.3e} "
          f"(tolerance {TOL_E2E:g}), largest rise {np.diff(obj).max() / obj[0]:.3e} of the first")
    assert rel.max() <= TOL_E2E
    assert np.diff(obj).max() <= 1e-6 * obj[0]
    at = tuple(int(v) for v in np.unravel_index(int(vol.argmax()), tuple(vol.shape)))
    assert at == c["voxel"] and float(vol.min()) >= 0.0
    fista, fobj = LCT.lct_solve(rows, op, iterations=30, step=step, accelerate=True)
    final = lambda v: 0.5 * float((op.forward(v) - rows).double().square().sum())
    lw, fi = final(vol), final(fista)
    print(f"  after 30 steps: Landweber {lw:.6g} (float64 {s['final'][0]:.6g}), FISTA {fi:.6g} (float64 "
          f"{s['final'][1]:.6g})")
    assert fi < lw and float(fista.min()) >= 0.0
    at = tuple(int(v) for v in np.unravel_index(int(fista.argmax()), tuple(fista.shape)))
    assert at == c["voxel"]
    # the default step is 1 / op.norm(); x0 and nonneg reach the loop
    again, obj2 = LCT.lct_solve(rows, op, iterations=2)
    assert abs(float(obj2[1]) / obj[1] - 1.0) <= 1e-4
    warm, obj3 = LCT.lct_solve(rows, op, iterations=1, step=step, x0=vol, nonneg=False)
    assert float(obj3[0]) == lw or abs(float(obj3[0]) / lw - 1.0) <= 1e-6
    with pytest.raises(ValueError):
        LCT.lct_solve(rows[:-1].contiguous(), op)
    with pytest.raises(ValueError):
        LCT.lct_solve(rows, op, x0=vol[:-1].contiguous())


def test_project_is_differentiable_through_the_adjoint():
    c, r0, dr, vol, rows = _inputs("5x7x17_r3")
    op = _operator(c, r0, dr, power=-3, nv=23)
    v = _dev(vol).requires_grad_(True)
    g = _dev(rows)
    out = op.project(v)
    assert out.requires_grad and torch.equal(out.detach(), op.forward(_dev(vol)))
    (grad,) = torch.autograd.grad(out, v, g)
    assert torch.equal(grad, op.adjoint(g))


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


def test_voxel_fit_step_through_the_operator(tmp_path):
    from nlosgr.data import make_data_kwargs
    from nlosgr.init import sample_from_volume
    from nlosgr.loss import loss as fused_loss
    from nlosgr.voxel_fit import VoxelFitStep, fit_capture, model_from_points
    from nlosgr.voxelize import voxelize
    c = CAPTURE
    _write_capture(tmp_path / "cap.mat")
    dk, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    out = LCT.lct_capture(dk, 20, 84)
    np.random.seed(3)
    torch.manual_seed(3)
    pts, rho = sample_from_volume(SimpleNamespace(init_gaussian_num=200), dk, out["volume"], out["grid"])
    model = model_from_points(pts, rho, c["sx"])
    step = fit_capture(dk, model, None, 20, 84, falloff=3, projector="lct", preset="cuda", keep_grads=True)
    op = step.operator
    assert isinstance(op, LCT.LctOperator) and step.grid.shape == op.volume_shape == (16, 64, 16) and step.walls is None
    pred = step.project(voxelize(model, step.grid, step.cam, preset="cuda", want_density=False)[1])
    step.volume_scale = float((pred.double() * step.rows.double()).sum()) / float(pred.double().square().sum())
    assert step.volume_scale > 0 and step.volume_scale != 1.0
    losses = [step()[0].clone()]
    g_rows = fused_loss(step.rows_pred, step.rows, step.gt_times, irf=step.irf, kind=step.loss_kind,
                        rate_floor=step.rate_floor)[1]
    assert torch.equal(step.rows_pred, op.forward(step.volume).mul_(step.volume_scale))
    assert torch.equal(step.grad_volume, op.adjoint(g_rows).mul_(step.volume_scale))
    for _ in range(20):
        losses.append(step()[0].clone())
    first, last = float(losses[0]), float(losses[-1])
    print(f"VoxelFitStep(operator=): loss {first:.6g} -> {last:.6g} after 20 steps, volume_scale {step.volume_scale:.4g}")
    assert last < first
    with pytest.raises(ValueError, match="rows must be"):
        VoxelFitStep(model, step.grid, step.cam, rows=step.rows[:-1].contiguous(), operator=op)


def test_lct_solve_capture_shuffled_unshuffled_and_cropped(tmp_path):
    from nlosgr.data import make_data_kwargs
    c = CAPTURE
    rows, xs, zs = _write_capture(tmp_path / "cap.mat")
    torch.manual_seed(6)
    dks, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=True)
    dku, *_ = make_data_kwargs(str(tmp_path / "cap.mat"), DEV, shuffle=False)
    assert not torch.equal(dks["index"], dku["index"])
    full = LCT.lct_solve_capture(dku, 20, 84, iterations=8, crop=False)
    assert sorted(full) == ["depth", "front", "grid", "objective", "volume"]
    assert full["volume"].shape == full["grid"].shape == (16, 64, 16) and full["objective"].shape == (8,)
    at = tuple(int(v) for v in np.unravel_index(int(full["volume"].argmax()), (16, 64, 16)))
    assert at == c["voxel"]
    again = LCT.lct_solve_capture(dks, 20, 84, iterations=8, crop=False)
    assert torch.equal(full["volume"], again["volume"])               # (the objective sums the rows in their own order)
    assert torch.allclose(full["objective"], again["objective"], rtol=1e-12, atol=0.0)
    # the volume is lct_solve's for the capture's rows times r^3
    cdt = float(dku["c"]) * float(dku["deltaT"])
    radii = 20 * cdt + cdt * torch.arange(64, dtype=torch.float64, device=DEV)
    scaled = (_dev(rows).double() * radii.pow(3.0)[None]).float()
    op = LCT.LctOperator(16, 16, c["sx"], c["sz"], 20 * cdt, cdt, 64, device=DEV)
    want, _ = LCT.lct_solve(scaled, op, iterations=8, accelerate=True)
    assert torch.equal(full["volume"], want)
    lw = LCT.lct_solve_capture(dku, 20, 84, iterations=8, accelerate=False, falloff=2, power=1, nv=100, crop=False)
    op = LCT.LctOperator(16, 16, c["sx"], c["sz"], 20 * cdt, cdt, 64, power=1, nv=100, device=DEV)
    want, _ = LCT.lct_solve((_dev(rows).double() * radii.pow(2.0)[None]).float(), op, iterations=8)
    assert torch.equal(lw["volume"], want) and not torch.equal(lw["volume"], full["volume"])
    # crop: exactly the block of the voxels inside the volume box
    inside = []
    for t, p in zip(full["grid"].tables, BOX["position"]):
        ok = np.nonzero((t.numpy() >= p - BOX["size"] / 2) & (t.numpy() <= p + BOX["size"] / 2))[0]
        inside.append((int(ok[0]), int(ok[-1]) + 1))
    (x0, x1), (y0, y1), (z0, z1) = inside
    assert (x1 - x0, y1 - y0, z1 - z0) == (10, 31, 10)
    for dk in (dku, dks):
        crop = LCT.lct_solve_capture(dk, 20, 84, iterations=8)
        assert torch.equal(crop["volume"], full["volume"][x0:x1, y0:y1, z0:z1]) and crop["volume"].is_contiguous()
        assert crop["grid"].shape == (10, 31, 10) and torch.equal(crop["grid"].ys, full["grid"].ys[y0:y1])
        assert crop["front"].shape == crop["depth"].shape == (10, 10)
    _write_capture(tmp_path / "nc.mat", lasers=True)
    dk, *_ = make_data_kwargs(str(tmp_path / "nc.mat"), DEV, shuffle=False)
    with pytest.raises(NotImplementedError, match="nlosgr.phasor"):
        LCT.lct_solve_capture(dk, 20, 84)
    bent = dict(dku)
    pos = dku["camera_grid_positions"].clone()
    pos[0] = pos[0] * pos[0].abs()                                 # non-uniform spacing
    bent["camera_grid_positions"] = pos
    with pytest.raises(ValueError, match="lattice"):
        LCT.lct_solve_capture(bent, 20, 84)


def test_command_line_iterations(tmp_path):
    from nlosgr.data import make_data_kwargs
    _write_capture(tmp_path / "cap.mat")
    cap = str(tmp_path / "cap.mat")
    plain, zero, solved = (str(tmp_path / n) for n in ("plain.npz", "zero.npz", "solved.npz"))
    base = [cap, "--start", "20", "--end", "84", "--snr", "2", "--nv", "96"]
    LCT.main(base + ["--out", plain])
    LCT.main(base + ["--iterations", "0", "--out", zero])
    dk, *_ = make_data_kwargs(cap, DEV, shuffle=False)
    today = LCT.lct_capture(dk, 20, 84, snr=2.0, nv=96)
    keys = sorted(["density", "albedo", "front", "depth", "xs", "ys", "zs", "cam"])
    a, b = np.load(plain), np.load(zero)
    assert sorted(a.files) == sorted(b.files) == keys
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["density"], today["volume"].cpu().numpy())
    assert np.array_equal(a["front"], today["front"].cpu().numpy())
    LCT.main(base + ["--iterations", "6", "--no-accelerate", "--falloff", "2", "--out", solved])
    z = np.load(solved)
    assert sorted(z.files) == sorted(keys + ["objective"]) and z["objective"].shape == (6,)
    want = LCT.lct_solve_capture(dk, 20, 84, falloff=2.0, power=0, iterations=6, accelerate=False, nv=96)
    assert np.array_equal(z["density"], want["volume"].cpu().numpy()) and np.array_equal(z["albedo"], z["density"])
    assert np.array_equal(z["objective"], want["objective"].cpu().numpy())
    assert np.array_equal(z["ys"], a["ys"]) and (np.diff(z["objective"]) < 0).all()
