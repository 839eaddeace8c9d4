"""GPU checks of the primal-dual passes (include/nlosgr.h "Primal-dual passes": nlosgr_prox_rows, nlosgr_tv_dual,
nlosgr_tv_primal; csrc/nlosgr_prox.hip; nlosgr.prox) against the float64 oracle of tests/prox_oracle.py, which starts
from the fp32 inputs the kernels get.

Shapes (W, nr, H): (1,1,1) all axes of extent 1; (2,2,2) the smallest volume with neighbours; (7,17,5) all odd;
(16,9,1) H = 1; (1,5,3) W = 1; (3,1,4) nr = 1; (2,3,70) H > 64; (3,300,2) nr > 256; (5,40,33) a plane of 1320
elements, no multiple of 64, over two workgroups; and (2,2,1024), the longest halo (H = 1024) the LDS image holds.
Inputs are signed and seeded, the axis weights unequal (1.5, 0.75, 2.25).  Every array handed to a pass is a window
of a larger NaN-filled buffer, which must stay NaN around it.

Derived tolerances (u = 2^-24), per element, relative to the sum of the absolute terms:
  gradient (tv = inf, p = 0, sigma = 1)   (1 + u)^2 - 1: the subtraction and the product; the fma with 1 and 0 is exact.
  dual update                             (1 + u)^9 - 1: the three roundings of u_k = fma(sigma, a (x' - x), p), and where
                                          it projects the product, two fma, the square root, the division and the final
                                          product (6); the sum of absolute terms is S_k = sigma a_k (|x'| + |x|) + |p_k|
                                          inside the ball and (tv / n) S_k + |p_k| |S|_2 / n outside.
  primal update x+                        (1 + u)^7 - 1 of |x| + tau (|g| + sum_k a_k (|p_k[i - e_k]| + |p_k[i]|) + l1):
                                          subtraction, product, two sums, the sum with g, the fma, the threshold.
  xbar                                    one rounding of 2 x+ - x with the pass's own x+.
  adjoint identity on the device          (1 + u)^4 - 1 of sum |a o grad|x|| . |p| (2 roundings on one side, 4 on the
                                          other), float64 dot products.
  MSE prox                                (1 + u)^4 - 1 of (|q| + sigma |z| + sigma |h|) / (1 + sigma).
  partial sums                            1e-12 relative: they are formed in double.

Measured tolerance.  The Poisson prox is checked over d in {0, 1e-3, 1, 3.7e7} (and the NULL table), h in {0, 3, 1e5},
the pass's own argument u = q + sigma z in {-1e6, -2, 0.999, 1, 1.001, 5, 300} and sigma in {0.37, 30}, and on dense
seeded rows with gt_times 2.5 and rate_floor 0.3, as a fraction of |u| + sigma y' / d + sigma eps / d, the absolute
terms of d (s - s' y') = u + sigma eps / d - sigma y' / d, against the float64 closed form (whose own optimality
residual is <= 1.2e-16 there).  Under this scale the textbook form d (1 + s - D) / 2 evaluated in fp32 is wrong by 1.0
at d = 3.7e7 (it returns 0 for q = 1.001).  The tolerance is 4 x the worst value measured on the MI355X, one digit up,
and never above 2e-5, the cap of test_gpu_lct.py:

    Poisson prox   measured 1.60e-7 (the seeded rows; 1.36e-7 at d = 3.7e7, h = 3, u = 1.001, sigma = 0.37 on the grid)
                   4 x = 6.42e-7   tolerance 7e-7

The derived checks reach at most 1.88 u (gradient, bound 2 u), 2.42 u (dual update, bound 9 u), 2.60 u (x+, bound 7 u),
1.00 u (xbar, bound 1 u), 2.33 u (the transpose alone, bound 4 u), 0.17 u (adjoint identity, bound 4 u) and 1.98 u (MSE
prox, bound 4 u); every emitted sum equals its float64 value to the 15 digits printed.

In every case q < d, and q = 0 where d = 0.  Run with -s for the measured figures."""
import numpy as np
import pytest
import torch

import prox_oracle as PO
from nlosgr import prox as PX

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
CAP = 2e-5
TOL_POISSON = 7e-7
SHAPES = [(1, 1, 1), (2, 2, 2), (7, 17, 5), (16, 9, 1), (1, 5, 3), (3, 1, 4), (2, 3, 70), (3, 300, 2), (5, 40, 33),
          (2, 2, 1024)]
WEIGHTS = (1.5, 0.75, 2.25)
PAD = 64                                               # floats of NaN on either side of every array

assert TOL_POISSON <= CAP


def bound(k):
    return (1.0 + U) ** k - 1.0


class Framed:
    """A float32 tensor of `values` inside a NaN frame: .t is the window the pass gets (offset: floats before it)."""

    def __init__(self, values, offset=PAD):
        values = np.ascontiguousarray(values, dtype=np.float32)
        self.buf = torch.full((offset + values.size + PAD,), float("nan"), device=DEV)
        self.offset, self.n = offset, values.size
        self.t = self.buf[offset:offset + values.size].view(values.shape)
        self.t.copy_(torch.from_numpy(values))

    def get(self):
        """The window as float64 numpy; the frame must still be NaN."""
        b = self.buf.cpu().numpy()
        assert np.isnan(b[:self.offset]).all() and np.isnan(b[self.offset + self.n:]).all(), "a pass wrote outside"
        return self.t.cpu().numpy().astype(np.float64)


def _inputs(shape, seed=0):
    g = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + shape[2] + seed)
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    return f(*shape), f(*shape), f(*shape), f(3, *shape)          # x, xbar, g, p


def _abs_gradient(x, a):
    """a_k (|x'| + |x|) where the difference exists, else 0: the absolute terms of the gradient."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    s = np.zeros((3,) + x.shape)
    s[0, :-1] = a[0] * (x[1:] + x[:-1])
    s[1, :, :-1] = a[1] * (x[:, 1:] + x[:, :-1])
    s[2, :, :, :-1] = a[2] * (x[:, :, 1:] + x[:, :, :-1])
    return s


def _worst(err, scale):
    return float((err / np.where(scale > 0, scale, 1.0)).max())


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradient_alone_and_the_emitted_sums(shape):
    x = _inputs(shape)[1]
    xf = Framed(x)
    got = PX.tv_gradient(xf.t, WEIGHTS)
    assert got.shape == (3,) + shape and got.dtype == torch.float32
    xf.get()
    want, scale = PO.grad(x, WEIGHTS), _abs_gradient(x, WEIGHTS)
    g = got.cpu().numpy().astype(np.float64)
    assert (g[scale == 0] == 0).all()                             # the last index of every axis, and extent-1 axes
    worst = _worst(np.abs(g - want), scale)
    print(f"{shape}: gradient worst error {worst / U:.2f} u (bound {bound(2) / U:.2f} u)")
    assert worst <= bound(2)
    assert torch.equal(got, PX.tv_gradient(xf.t, WEIGHTS))
    # the sums the dual pass emits, at any sigma and tv
    p = Framed(_inputs(shape)[3])
    sums = PX.tv_dual_step(p.t, xf.t, 0.3, 0.5, WEIGHTS).cpu().numpy()
    assert sums.shape == (2,) and sums.dtype == np.float64
    tv64, l164 = PO.tv_sum(x, WEIGHTS), float(np.abs(x.astype(np.float64)).sum())
    print(f"{shape}: TV {sums[0]:.15g} (float64 {tv64:.15g}), L1 {sums[1]:.15g} (float64 {l164:.15g})")
    assert abs(sums[0] - tv64) <= 1e-12 * tv64 and abs(sums[1] - l164) <= 1e-12 * l164


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_dual_update_and_projection(shape):
    _, xbar, _, p = _inputs(shape)
    sigma = 0.37
    u64 = p.astype(np.float64) + sigma * PO.grad(xbar, WEIGHTS)
    S = sigma * _abs_gradient(xbar, WEIGHTS) + np.abs(p.astype(np.float64))
    n64 = PO.norm3(u64)
    worst_all = 0.0
    for tv in (float(np.median(n64)), float(n64.max()) * 2.0, float(n64.min()) * 0.5, float("inf")):
        xf, pf = Framed(xbar), Framed(p)
        PX.tv_dual_step(pf.t, xf.t, sigma, tv, WEIGHTS)
        got, want = pf.get(), PO.project(u64, tv)
        assert np.array_equal(xf.get(), xbar.astype(np.float64))
        ns = np.where(n64 > 0, n64, 1.0)
        outside = n64 > tv
        with np.errstate(invalid="ignore"):
            scale = np.where(outside[None], (tv / ns)[None] * S + np.abs(want) * (PO.norm3(S) / ns)[None], S)
        worst = _worst(np.abs(got - want), scale)
        worst_all = max(worst_all, worst)
        gn = PO.norm3(got)
        assert (gn <= tv * (1.0 + 4.0 * U)).all()
        print(f"{shape} tv {tv:.4g}: {int(outside.sum())} of {outside.size} projected, worst error {worst / U:.2f} u "
              f"(bound {bound(9) / U:.2f} u)")
        again = Framed(p)
        PX.tv_dual_step(again.t, xf.t, sigma, tv, WEIGHTS)
        assert torch.equal(again.t, pf.t)
    assert worst_all <= bound(9)
    # tv = 0 writes zeros
    pf = Framed(p)
    PX.tv_dual_step(pf.t, Framed(xbar).t, sigma, 0.0, WEIGHTS)
    assert (pf.get() == 0).all()


def test_projection_at_the_ball():
    """|u| < tv, = tv and > tv with exact fp32 norms: (3, 4, 0) c has the norm 5 c.  xbar = 0, so u = p."""
    shape = (2, 2, 2)
    p = np.zeros((3,) + shape, dtype=np.float32)
    c = np.array([0.5, 1.0, 2.0, 4.0, 0.25, 1.0, 1.0, 8.0], dtype=np.float32).reshape(shape)
    p[0], p[1] = 3.0 * c, 4.0 * c
    pf = Framed(p)
    PX.tv_dual_step(pf.t, Framed(np.zeros(shape)).t, 1.0, 5.0, WEIGHTS)
    got = pf.get()
    inside = (5.0 * c <= 5.0)
    assert inside.sum() == 5 and (5.0 * c == 5.0).sum() == 3
    assert np.array_equal(got[:, inside], p.astype(np.float64)[:, inside])          # <= tv: the bits of u
    f = (np.float32(5.0) / (np.float32(5.0) * c)).astype(np.float32)
    want = (p * f[None]).astype(np.float64)
    assert np.array_equal(got[:, ~inside], want[:, ~inside])                        # > tv: u (tv / n), one division


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_primal_update(shape):
    x, _, g, p = _inputs(shape)
    tau = 0.21
    a = WEIGHTS
    absdiv = PO.grad_t_abs(p, a)
    u64 = x.astype(np.float64) - tau * (g.astype(np.float64) + PO.grad_t(p, a))
    worst_all = 0.0
    for l1, nonneg in ((0.0, True), (0.9, True), (0.9, False), (0.0, False)):
        thr = tau * float(np.float32(l1))
        xf, bf, gf, pf = Framed(x), Framed(np.full(shape, np.nan)), Framed(g), Framed(p)
        PX.tv_primal_step(xf.t, bf.t, gf.t, pf.t, tau, l1, a, nonneg)
        xp, xb = xf.get(), bf.get()
        assert np.array_equal(gf.get(), g.astype(np.float64)) and np.array_equal(pf.get(), p.astype(np.float64))
        want = PO.shrink(u64, thr, nonneg)
        scale = np.abs(x.astype(np.float64)) + tau * (np.abs(g.astype(np.float64)) + absdiv) + thr
        worst = _worst(np.abs(xp - want), scale)
        worst_all = max(worst_all, worst)
        if nonneg:
            assert (xp >= 0).all() and (xp.size < 100 or ((xp == 0).any() and (xp > 0).any()))   # the clamp acts
        else:
            assert ((xp < 0).any() and (xp > 0).any()) or xp.size < 4
            if l1 > 0 and xp.size > 100:
                assert (xp == 0).any()                            # the dead zone of the soft threshold
        bar = 2.0 * xp - x.astype(np.float64)
        wb = _worst(np.abs(xb - bar), 2.0 * np.abs(xp) + np.abs(x.astype(np.float64)))
        print(f"{shape} l1 {l1} nonneg {nonneg}: x+ worst error {worst / U:.2f} u (bound {bound(7) / U:.2f} u), "
              f"xbar {wb / U:.2f} u (bound 1 u)")
        assert wb <= bound(1)
        x2, b2 = Framed(x), Framed(np.full(shape, np.nan))
        PX.tv_primal_step(x2.t, b2.t, gf.t, pf.t, tau, l1, a, nonneg)
        assert torch.equal(x2.t, xf.t) and torch.equal(b2.t, bf.t)
    assert worst_all <= bound(7)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_adjoint_identity_on_the_device(shape):
    x, _, _, p = _inputs(shape, seed=3)
    xd, pd = Framed(x), Framed(p)
    gx, dp = PX.tv_gradient(xd.t, WEIGHTS), PX.tv_divergence(pd.t, WEIGHTS)
    assert dp.shape == shape
    lhs = float((gx.double() * pd.t.double()).sum())
    rhs = float((xd.t.double() * dp.double()).sum())
    scale = float((_abs_gradient(x, WEIGHTS) * np.abs(p.astype(np.float64))).sum())
    want = PO.grad_t(p, WEIGHTS)
    err = _worst(np.abs(dp.cpu().numpy().astype(np.float64) - want), PO.grad_t_abs(p, WEIGHTS))
    print(f"{shape}: <grad x, p> - <x, grad^T p> = {lhs - rhs:.3e} of {scale:.3e}; grad^T worst error {err / U:.2f} u")
    assert abs(lhs - rhs) <= bound(4) * scale
    assert err <= bound(4)


def test_an_unaligned_window_gives_the_same_bits():
    """(5, 40, 33): its plane is a multiple of 4, so aligned arrays take the 16-byte accesses and a window that
    starts 3 floats into its buffer the 4-byte ones."""
    shape = (5, 40, 33)
    x, xbar, g, p = _inputs(shape)
    out = []
    for off in (PAD, 3):
        xf, bf, gf, pf = (Framed(v, off) for v in (x, xbar, g, p))
        sums = PX.tv_dual_step(pf.t, bf.t, 0.37, 1.1, WEIGHTS)
        PX.tv_primal_step(xf.t, bf.t, gf.t, pf.t, 0.21, 0.4, WEIGHTS, True)
        for f in (xf, bf, gf, pf):
            f.get()
        out.append((sums.clone(), xf.t.clone(), bf.t.clone(), pf.t.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def _rows(H, W, nr, seed):
    g = np.random.default_rng(seed)
    f = lambda: g.standard_normal((H * W, nr)).astype(np.float32)
    return f(), f(), f()


@pytest.mark.parametrize("H,W,nr", [(1, 1, 1), (3, 5, 7), (4, 16, 67), (5, 3, 300)])
def test_mse_prox(H, W, nr):
    """4 x 16 x 67 = 4288 elements: two workgroups, the second partial."""
    q, z, h = _rows(H, W, nr, 11)
    sigma = 0.37
    qf, zf, hf = Framed(q), Framed(z), Framed(h)
    F = float(PX.prox_rows(qf.t, zf.t, hf.t, H, W, sigma))
    got = qf.get()
    assert np.array_equal(zf.get(), z.astype(np.float64)) and np.array_equal(hf.get(), h.astype(np.float64))
    q64, z64, h64 = (v.astype(np.float64) for v in (q, z, h))
    s32 = float(np.float32(sigma))
    want = PO.prox_mse(q64 + s32 * z64, h64, s32)
    scale = (np.abs(q64) + s32 * np.abs(z64) + s32 * np.abs(h64)) / (1.0 + s32)
    worst = _worst(np.abs(got - want), scale)
    F64 = PO.data_term(z, h)
    print(f"{H}x{W}x{nr}: MSE prox worst error {worst / U:.2f} u (bound {bound(4) / U:.2f} u); F {F:.15g} "
          f"(float64 {F64:.15g})")
    assert worst <= bound(4) and abs(F - F64) <= 1e-12 * F64
    again = Framed(q)
    assert float(PX.prox_rows(again.t, zf.t, hf.t, H, W, sigma)) == F and torch.equal(again.t, qf.t)
    with pytest.raises(ValueError, match="exposure"):
        PX.prox_rows(again.t, zf.t, hf.t, H, W, sigma, exposure=torch.ones(nr, device=DEV))


D_TABLE = (0.0, 1e-3, 1.0, 3.7e7)
H_VALUES = (0.0, 3.0, 1e5)
U_VALUES = (-1e6, -2.0, 0.999, 1.0, 1.001, 5.0, 300.0)


@pytest.mark.parametrize("table", [True, False], ids=["exposure", "null"])
def test_poisson_prox(table):
    """Rows [21, 4]: one row per (h, u) pair, one column per d of the table (d = 1 everywhere without it)."""
    nr, Hl, Wl = len(D_TABLE), len(H_VALUES), len(U_VALUES)
    e = np.array(D_TABLE, dtype=np.float32)
    d = e.astype(np.float64) if table else np.ones(nr)
    hh, uu = (v.reshape(-1) for v in np.meshgrid(H_VALUES, U_VALUES, indexing="ij"))
    h = np.repeat(hh[:, None], nr, axis=1).astype(np.float32)
    worst_all, where = 0.0, None
    for sigma in (0.37, 30.0):
        s32 = float(np.float32(sigma))
        # u = q + sigma z: split the target between the two
        q = np.repeat((0.25 * uu)[:, None], nr, axis=1).astype(np.float32)
        z = ((np.repeat(uu[:, None], nr, axis=1) - q.astype(np.float64)) / s32).astype(np.float32)
        u64 = q.astype(np.float64) + s32 * z.astype(np.float64)
        qf, zf, hf = Framed(q), Framed(z), Framed(h)
        ef = Framed(e) if table else None
        kw = dict(loss="poisson", exposure=ef.t if table else None, gt_times=1.0, rate_floor=1.0)
        F = float(PX.prox_rows(qf.t, zf.t, hf.t, Hl, Wl, sigma, **kw))
        got = qf.get()
        if table:
            assert np.array_equal(ef.get(), e.astype(np.float64))
        want = PO.prox_poisson(u64, h, s32, d, 1.0, 1.0)
        yp = PO.counts64(h, 1.0, 1.0)
        live = np.broadcast_to(d > 0, got.shape)
        ds = np.where(d > 0, d, 1.0)[None]
        err = np.abs(got - want) / (np.abs(u64) + s32 * yp / ds + s32 * 1.0 / ds)
        assert (got[~live] == 0).all() and (got[live] < np.broadcast_to(d, got.shape)[live]).all()
        res = PO.prox_poisson_residual(want, u64, h, s32, d, 1.0, 1.0).max()
        assert res <= 5e-12
        i = np.unravel_index(int(np.where(live, err, 0).argmax()), err.shape)
        print(f"sigma {sigma} table {table}: Poisson prox worst error {err[live].max():.3e} at d = {d[i[1]]:g}, "
              f"h = {h[i]:g}, u = {u64[i]:.6g} (tolerance {TOL_POISSON:g}); float64 residual {res:.1e}")
        if err[live].max() > worst_all:
            worst_all, where = float(err[live].max()), (float(d[i[1]]), float(h[i]), float(u64[i]), sigma)
        F64 = PO.data_term(z, h, "poisson", d, 1.0, 1.0)
        print(f"    F {F:.15g} (float64 {F64:.15g})")
        assert abs(F - F64) <= 1e-12 * F64
        again = Framed(q)
        assert float(PX.prox_rows(again.t, zf.t, hf.t, Hl, Wl, sigma, **kw)) == F and torch.equal(again.t, qf.t)
    print(f"Poisson prox, table {table}: worst {worst_all:.3e} at (d, h, u, sigma) = {where}")
    assert worst_all <= TOL_POISSON


def test_poisson_prox_on_seeded_rows_with_gt_times():
    """Dense signed z and q, counts h >= 0, an exposure that falls with the bin, gt_times and a rate floor that are
    not 1; 4 x 16 x 67 elements over two workgroups."""
    H, W, nr = 4, 16, 67
    q, z, h = _rows(H, W, nr, 12)
    h = np.abs(h * 40.0).astype(np.float32)
    h[::3] = 0.0
    e = (1.0 / (0.2 + 0.05 * np.arange(nr)) ** 3).astype(np.float32)
    e[0] = 0.0
    sigma, gt, eps = 0.6, 2.5, 0.3
    s32, g32, e32 = (float(np.float32(v)) for v in (sigma, gt, eps))
    qf = Framed(q)
    F = float(PX.prox_rows(qf.t, Framed(z).t, Framed(h).t, H, W, sigma, "poisson", Framed(e).t, gt, eps))
    got = qf.get()
    d = e.astype(np.float64)
    u64 = q.astype(np.float64) + s32 * z.astype(np.float64)
    want = PO.prox_poisson(u64, h, s32, d, g32, e32)
    ds = np.where(d > 0, d, 1.0)[None]
    err = np.abs(got - want) / (np.abs(u64) + s32 * PO.counts64(h, g32, e32) / ds + s32 * e32 / ds)
    F64 = PO.data_term(z, h, "poisson", d, g32, e32)
    print(f"seeded rows: Poisson prox worst error {err.max():.3e} (tolerance {TOL_POISSON:g}); F {F:.15g} "
          f"(float64 {F64:.15g})")
    assert (got[:, 0] == 0).all() and (got[:, 1:] < d[None, 1:]).all()
    assert err.max() <= TOL_POISSON and abs(F - F64) <= 1e-12 * F64


def test_poisson_prox_exposure_whose_square_underflows():
    """d d is 0 in fp32 below d = 2^-75: the pass treats such an entry as d = 0 (q = 0), never inf or NaN."""
    H, W, nr = 2, 3, 4
    q, z, h = _rows(H, W, nr, 13)
    e = np.array([1e-30, 2.0 ** -76, 1e-6, 1.0], dtype=np.float32)
    qf = Framed(q)
    F = float(PX.prox_rows(qf.t, Framed(z).t, Framed(np.abs(h)).t, H, W, 0.5, "poisson", Framed(e).t))
    got = qf.get()
    assert np.isfinite(F) and np.isfinite(got).all() and (got[:, :2] == 0).all() and (got[:, 2:] != 0).all()
    assert (got[:, 2:] < e.astype(np.float64)[None, 2:]).all()
