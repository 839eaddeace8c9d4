"""The primal-dual passes without a GPU: the five new entry points and their host-side validation, the float64
oracle's own identities (tests/prox_oracle.py: the gradient's transpose, the optimality condition of the Poisson prox,
a Chambolle-Pock objective that settles), the norm's safety factor, the Python surface's refusals, the command line's
new flags, and lct_solve_capture's default path."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fk_oracle as FO
import lct_oracle as LO
import lct_op_oracle as OO
import prox_oracle as PO
from nlosgr import lct as LCT
from nlosgr import prox as PX

NEW = ("nlosgr_prox_rows_partials", "nlosgr_prox_rows", "nlosgr_tv_dual_partials", "nlosgr_tv_dual", "nlosgr_tv_primal")
INF, NAN = float("inf"), float("nan")


def test_library_carries_the_entry_points():
    from nlosgr import _lib
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.nlosgr_abi_version() == 13 and _lib.ABI_VERSION == 13
    import nlosgr
    for name in ("primal_dual", "prox_rows", "tv_dual_step", "tv_primal_step", "tv_gradient", "tv_divergence"):
        assert getattr(nlosgr, name) is getattr(PX, name) and name in nlosgr.__all__, name
    assert nlosgr.lct_solve_pd is LCT.lct_solve_pd and "lct_solve_pd" in nlosgr.__all__
    # one partial per 4096 row elements, two per 1024 plane elements of a wall column
    assert lib.nlosgr_prox_rows_partials(4, 16, 67) == 2 and lib.nlosgr_prox_rows_partials(1, 1, 1) == 1
    assert lib.nlosgr_tv_dual_partials(5, 40, 33) == 2 * 5 * 2 and lib.nlosgr_tv_dual_partials(1, 1, 1) == 2
    assert lib.nlosgr_prox_rows_partials(0, 1, 1) == 0 and lib.nlosgr_tv_dual_partials(1, 1025, 1) == 0


def test_entry_points_validate_on_the_host():
    """Every check runs before any launch and reports through nlosgr_last_error (no GPU; the fake non-null
    pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    P = lambda a: ctypes.c_void_p(a)
    z, h, q, part, e = P(1 << 20), P(2 << 20), P(3 << 20), P(4 << 20), P(5 << 20)
    err = lib.nlosgr_last_error

    def rows(z=z, h=h, e=None, H=4, W=6, nr=8, kind=0, gt=1.0, eps=1.0, sigma=0.5, q=q, part=part):
        return lib.nlosgr_prox_rows(z, h, e, H, W, nr, kind, gt, eps, sigma, q, part, None)

    x, xbar, g, p = P(1 << 20), P(2 << 20), P(3 << 20), P(4 << 20)

    def dual(xbar=xbar, W=6, nr=8, H=4, a=(1.0, 1.0, 1.0), sigma=0.5, tv=1.0, p=p, part=part):
        return lib.nlosgr_tv_dual(xbar, W, nr, H, a[0], a[1], a[2], sigma, tv, p, part, None)

    def primal(g=g, p=p, W=6, nr=8, H=4, a=(1.0, 1.0, 1.0), tau=0.5, l1=0.1, nonneg=1, x=x, xbar=xbar):
        return lib.nlosgr_tv_primal(g, p, W, nr, H, a[0], a[1], a[2], tau, l1, nonneg, x, xbar, None)

    for fn in (rows, dual, primal):
        for bad in (dict(H=0), dict(W=-1), dict(H=1025), dict(W=1025), dict(nr=0), dict(nr=1025)):
            assert fn(**bad) == 1 and b"1..1024" in err(), (fn.__name__, bad)
    for bad in (0.0, -1.0, INF, NAN):
        assert rows(sigma=bad) == 1 and b"sigma" in err(), bad
        assert dual(sigma=bad) == 1 and b"sigma" in err(), bad
        assert primal(tau=bad) == 1 and b"tau" in err(), bad
    for bad in (-1e-3, NAN):
        assert dual(tv=bad) == 1 and b"tv" in err(), bad
    for bad in (-1e-3, INF, NAN):
        assert primal(l1=bad) == 1 and b"l1" in err(), bad
        for k in range(3):
            a = [1.0, 1.0, 1.0]
            a[k] = bad
            assert dual(a=a) == 1 and b"axis weights" in err(), (bad, k)
            assert primal(a=a) == 1 and b"axis weights" in err(), (bad, k)
    for kind in (-1, 2, 7):
        assert rows(kind=kind) == 1 and b"kind" in err(), kind
    for bad in (0.0, -1.0, INF, NAN):
        assert rows(kind=1, eps=bad) == 1 and b"rate_floor" in err(), bad
    assert rows(kind=0, e=e) == 1 and b"exposure" in err()
    for name in ("z", "h", "q", "part"):
        assert rows(**{name: None}) == 1 and b"null" in err(), name
    for name in ("xbar", "p", "part"):
        assert dual(**{name: None}) == 1 and b"null" in err(), name
    for name in ("g", "p", "x", "xbar"):
        assert primal(**{name: None}) == 1 and b"null" in err(), name
    # the aliasing the in-place scheme forbids: equal pointers, and ranges that overlap
    assert rows(q=z) == 1 and b"alias" in err()
    assert rows(q=P((1 << 20) + 64)) == 1 and b"alias" in err()
    assert rows(q=h) == 1 and b"alias" in err()
    assert rows(kind=1, e=P((3 << 20) + 16)) == 1 and b"alias" in err() and b"exposure" in err()
    for other in (z, h, q):
        assert rows(part=other) == 1 and b"alias" in err() and b"partials" in err()
    assert rows(kind=1, e=e, part=P((5 << 20) + 8)) == 1 and b"partials" in err()
    assert dual(p=xbar) == 1 and b"alias" in err()
    assert dual(part=xbar) == 1 and b"partials" in err()
    assert dual(part=P((4 << 20) + 1024)) == 1 and b"partials" in err()
    assert dual(xbar=P((4 << 20) + 2 * 4 * 192)) == 1 and b"alias" in err()       # inside p's third component
    assert primal(x=xbar) == 1 and b"alias" in err()
    assert primal(x=g) == 1 and b"alias" in err()
    assert primal(xbar=g) == 1 and b"alias" in err()
    assert primal(xbar=p) == 1 and b"alias" in err()
    assert primal(x=P((4 << 20) + 4 * 192)) == 1 and b"alias" in err()


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 2, 2), (7, 17, 5), (16, 9, 1), (1, 5, 3), (3, 1, 4), (5, 40, 33)])
def test_oracle_gradient_and_its_transpose(shape):
    g = np.random.default_rng(sum(shape))
    a = (1.5, 0.75, 2.25)
    x, p = g.standard_normal(shape), g.standard_normal((3,) + shape)
    gx, dp = PO.grad(x, a), PO.grad_t(p, a)
    scale = np.sqrt((gx * gx).sum() * (p * p).sum()) or 1.0
    assert abs((gx * p).sum() - (x * dp).sum()) <= 1e-12 * scale
    for k in range(3):                                                    # Neumann: 0 at the last index
        assert not np.moveaxis(gx[k], k, 0)[-1].any()
    assert PO.tv_sum(np.full(shape, 3.0), a) == 0.0
    # the squared norm of a o grad is at most 4 sum a^2: the bound behind the default steps
    v = g.standard_normal(shape)
    for _ in range(50):
        v = PO.grad_t(PO.grad(v, a), a)
        n = np.sqrt((v * v).sum())
        if n == 0:
            break
        v /= n
    assert n <= 4.0 * sum(w * w for w in a)


def test_oracle_projection_and_shrink():
    u = np.array([[3.0, 0.3, 0.0], [4.0, 0.4, 0.0], [0.0, 0.0, 0.0]]).reshape(3, 3, 1, 1)
    p = PO.project(u, 1.0)
    assert np.allclose(PO.norm3(p).reshape(-1), [1.0, 0.5, 0.0]) and np.array_equal(p[:, 1], u[:, 1])
    assert not PO.project(u, 0.0).any() and np.array_equal(PO.project(u, INF), u)
    v = np.array([-2.0, -0.5, 0.0, 0.5, 2.0])
    assert np.array_equal(PO.shrink(v, 1.0, True), [0, 0, 0, 0, 1.0])
    assert np.array_equal(PO.shrink(v, 1.0, False), [-1.0, 0, 0, 0, 1.0])


def test_oracle_poisson_prox_meets_its_optimality_condition():
    """d in 1e-3 .. 3.7e7 and 0, sigma in 1e-3 .. 1e2, u from far below to above the pole, h from 0 to 1e5: the
    residual of (1 - q')(s - q') = s' y' relative to its absolute terms is <= 5e-12, q < d, and q = 0 where d = 0."""
    g = np.random.default_rng(0)
    worst = 0.0
    d = np.array([0.0, 1e-3, 1e-2, 1.0, 30.0, 1e3, 3.7e7])
    for sigma in (1e-3, 1e-1, 0.37, 1.0, 30.0, 1e2):
        u = np.concatenate([g.standard_normal(40) * 10, -np.abs(g.standard_normal(20)) * 1e6, [0.999, 1.0, 1.001, 5.0, 300.0]])
        u = np.repeat(u[:, None], d.size, axis=1)
        h = np.abs(g.standard_normal(u.shape)) * np.array([0.0, 1.0, 1e3, 1e5])[g.integers(0, 4, u.shape)]
        for gt, eps in ((1.0, 1.0), (2.5, 0.3)):
            q = PO.prox_poisson(u, h, sigma, d, gt, eps)
            assert (q[:, 0] == 0).all() and (q[:, 1:] < d[None, 1:]).all()
            worst = max(worst, PO.prox_poisson_residual(q, u, h, sigma, d, gt, eps).max())
    print(f"Poisson prox: worst optimality residual {worst:.2e}")
    assert worst <= 5e-12
    # Moreau: u = prox_{sigma F*}(u) + sigma prox_{F / sigma}(u / sigma); the second prox minimises F(z) + sigma/2 (z - u/sigma)^2
    u, h, sigma, dd = np.array([[0.3]]), np.array([[4.0]]), 0.7, np.array([2.0])
    q = PO.prox_poisson(u, h, sigma, dd)
    z = np.linspace(-0.2, 5.0, 200001)
    cost = (dd * z + 1.0) - 5.0 * np.log(dd * z + 1.0) + 0.5 * sigma * (z - u[0, 0] / sigma) ** 2
    assert abs((u[0, 0] - q[0, 0]) / sigma - z[cost.argmin()]) <= 1e-4
    # and the data term is half the deviance: 0 at rho = y', positive elsewhere
    assert PO.data_term(np.array([[2.0]]), np.array([[4.0]]), "poisson", dd) == 0.0
    assert PO.data_term(np.array([[1.0]]), np.array([[4.0]]), "poisson", dd) > 0.0


def test_oracle_objective_settles():
    """5 x 7 x 17 lattice, a box phantom with noise, MSE, tv = 0.02 lambda0 and l1 = 0.01 lambda0: after 1600
    iterations the objective is the one after 800 to 2e-3 (float64: 9.9e-4), far below the start."""
    c = FO.DENSE["5x7x17_r3"]
    r0, dr = FO.window(c)
    op = OO.Operator64(c["H"], c["W"], c["sx"], c["sz"], r0, dr, c["nr"], 0)
    g = np.random.default_rng(5)
    truth = np.zeros((c["W"], c["nr"], c["H"]))
    truth[2:5, 6:11, 1:4] = 1.0
    h = (op.forward(truth) + 0.02 * g.standard_normal((c["H"] * c["W"], c["nr"]))).astype(np.float32)
    norm = LCT.NORM_SAFETY * PO.converged_norm(op)
    lam = PO.lambda0(op, h)
    tv, l1 = 0.02 * lam, 0.01 * lam
    root = np.sqrt(norm + 12.0)
    x, obj, terms = PO.primal_dual(op, h, 1600, norm, tv=tv, l1=l1, sigma=100.0 / root, tau=0.01 / root)
    print(f"objective {obj[0]:.6g} -> {obj[799]:.6g} (800) -> {obj[1599]:.6g} (1600)")
    assert abs(obj[799] / obj[1599] - 1.0) <= 2e-3 and obj[1599] < 0.2 * obj[0]
    assert np.allclose(obj, terms @ np.array([1.0, tv, l1]), rtol=1e-15) and (x >= 0).all()
    assert abs(PO.functional(op, x, h, tv, l1)[0] / obj[1599] - 1.0) <= 1e-3
    # above lambda0 the zero volume stays the minimiser
    x, obj, _ = PO.primal_dual(op, h, 20, norm, l1=1.001 * lam)
    assert not x.any()


def test_norm_safety_factor_covers_the_converged_power_iteration():
    """LctOperator.norm() stops after 8 iterations; in float64 the converged value is at most 1.000136 times that
    on the solver's test lattices, and NORM_SAFETY rounds it up."""
    worst = 0.0
    for name, nv, voxel in LO.PEAKS:
        c = LO.peak_case(name, voxel)
        r0, dr = FO.window(c)
        op = OO.Operator64(c["H"], c["W"], c["sx"], c["sz"], r0, dr, c["nr"], 0, nv)
        worst = max(worst, PO.converged_norm(op, 1e-12) / op.norm(8))
    print(f"converged / 8-iteration norm: worst {worst:.7f}")
    assert 1.0 <= worst <= 1.0002 < LCT.NORM_SAFETY == 1.01


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    rows, vol, p = torch.zeros(24, 8), torch.zeros(6, 8, 4), torch.zeros(3, 6, 8, 4)
    for call in (lambda: PX.prox_rows(rows, rows.clone(), rows.clone(), 4, 6, 0.5),
                 lambda: PX.tv_dual_step(p, vol, 0.5, 1.0),
                 lambda: PX.tv_primal_step(vol, vol.clone(), vol.clone(), p, 0.5),
                 lambda: PX.tv_gradient(vol),
                 lambda: PX.tv_divergence(p),
                 lambda: PX.primal_dual(rows, None, None, (6, 8, 4), 1.0, 3),
                 lambda: LCT.lct_solve_pd(rows, object.__new__(LCT.LctOperator))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="loss"):
        PX.prox_rows(rows, rows, rows, 4, 6, 0.5, loss="huber")
    with pytest.raises(ValueError, match="weights"):
        PX.default_steps(1.0, 1.0, (1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="norm_A"):
        PX.default_steps(0.0)
    with pytest.raises(TypeError, match="LctOperator"):
        LCT.lct_solve_pd(rows, None)
    # L = norm_A + 4 sum a^2, the second part with tv > 0 only
    assert PX.default_steps(5.0) == 1.0 / np.sqrt(5.0)
    assert PX.default_steps(5.0, 0.1, (1.0, 0.5, 2.0)) == 1.0 / np.sqrt(5.0 + 4.0 * 5.25)
    assert PX.default_steps(5.0, 0.1) == PO.default_step(5.0, 0.1)


def test_command_line_arguments(capsys):
    base = ["cap.mat", "--start", "20", "--end", "100", "--iterations", "12"]
    a = LCT.parse_args(base)
    assert (a.tv, a.l1, a.loss, a.rate_floor, a.gt_times, a.primal_dual) == (0.0, 0.0, "mse", 1.0, 1.0, False)
    a = LCT.parse_args(base + ["--loss", "mse", "--rate-floor", "2"])
    assert not a.primal_dual                                              # nothing that changes the solve
    a = LCT.parse_args(base + ["--tv", "0.02"])
    assert a.primal_dual and a.tv == 0.02 and a.iterations == 12 and a.power == 0 and a.falloff == 3.0
    a = LCT.parse_args(base + ["--l1", "0.1", "--loss", "poisson", "--rate-floor", "0.5", "--gt-times", "40"])
    assert a.primal_dual and (a.l1, a.loss, a.rate_floor, a.gt_times) == (0.1, "poisson", 0.5, 40.0)
    for extra in (["--tv", "-0.1"], ["--l1", "-1"], ["--tv", "inf"], ["--l1", "nan"], ["--loss", "huber"],
                  ["--rate-floor", "0"], ["--rate-floor", "-1"], ["--rate-floor", "inf"], ["--gt-times", "inf"]):
        with pytest.raises(SystemExit):
            LCT.parse_args(base + extra)
    for extra in (["--tv", "0.1"], ["--l1", "0.1"], ["--loss", "poisson"]):   # they belong to --iterations
        with pytest.raises(SystemExit):
            LCT.parse_args(["cap.mat", "--start", "20", "--end", "100"] + extra)
    capsys.readouterr()


def test_lct_solve_capture_default_path_is_lct_solve(monkeypatch):
    """With tv, l1 and loss at their defaults lct_solve_capture hands lct_solve the rows times r^falloff, as it
    always did, and never reaches the primal-dual solver; otherwise it hands lct_solve_pd tv and l1 times lambda0,
    and with loss="poisson" the raw rows and the exposure r^-falloff (0 at r = 0).  (CPU stand-ins; the GPU run is
    in test_gpu_lct_pd.py.)"""
    nr, cdt = 6, 0.5
    rows = torch.arange(2 * 3 * nr, dtype=torch.float32).reshape(6, nr) - 4.0
    lattice = SimpleNamespace(rows=rows, H=2, W=3, xs=None, zs=None, y0=0.0, perm=None, x_along="n", sx=0.1, sz=0.1,
                              r0=0.0, dr=cdt, nr=nr)
    calls = []

    class Op:
        def __init__(self, *a, **kw):
            self.kw = kw

        def grid(self, *a):
            return "grid"

        def adjoint(self, r):
            calls.append(("adjoint", r.clone()))
            return torch.full((3, nr, 2), 7.0)

    monkeypatch.setattr(LCT, "confocal_lattice", lambda dk, s, e, what: lattice)
    monkeypatch.setattr(LCT, "_gpu", lambda t, dtype, what: t)
    monkeypatch.setattr(LCT, "LctOperator", Op)
    monkeypatch.setattr(LCT, "capture_result", lambda dk, grid, vol, crop: {"volume": vol, "front": 0, "depth": 0, "grid": grid})
    monkeypatch.setattr(LCT, "lct_solve", lambda r, op, **kw: (calls.append(("ls", r, op.kw, kw)), ("vol", "obj"))[1])
    monkeypatch.setattr(LCT, "lct_solve_pd",
                        lambda r, op, **kw: (calls.append(("pd", r, op.kw, kw)), ("vol", "obj", "terms"))[1])
    radii = cdt * torch.arange(nr, dtype=torch.float64)
    out = LCT.lct_solve_capture({}, 0, nr, iterations=5, accelerate=False)
    assert sorted(out) == ["depth", "front", "grid", "objective", "volume"] and out["objective"] == "obj"
    (kind, r, opkw, kw), = calls
    assert kind == "ls" and kw == dict(iterations=5, accelerate=False) and opkw["power"] == 0
    assert torch.equal(r, (rows.double() * radii.pow(3.0)[None]).float())
    calls.clear()
    out = LCT.lct_solve_capture({}, 0, nr, iterations=5, tv=0.25, l1=0.5, weights=(1, 2, 3))
    assert sorted(out) == ["depth", "front", "grid", "lambda0", "objective", "terms", "volume"]
    assert out["lambda0"] == 7.0 and out["terms"] == "terms"
    (_, pulled), (kind, r, opkw, kw) = calls
    assert kind == "pd" and torch.equal(r, (rows.double() * radii.pow(3.0)[None]).float()) and torch.equal(pulled, r)
    assert (kw["tv"], kw["l1"], kw["loss"], kw["exposure"], kw["weights"]) == (1.75, 3.5, "mse", None, (1, 2, 3))
    calls.clear()
    out = LCT.lct_solve_capture({}, 0, nr, iterations=5, loss="poisson", falloff=2, rate_floor=0.5, gt_times=4.0)
    (_, pulled), (kind, r, opkw, kw) = calls
    assert kind == "pd" and torch.equal(r, rows) and opkw["power"] == 0              # the counts stay raw
    e = kw["exposure"]
    assert e.dtype == torch.float32 and e[0] == 0 and torch.equal(e[1:], radii[1:].pow(-2.0).float())
    assert torch.equal(pulled, (rows.double().mul(4.0).clamp(min=0) * (e.double() / 0.5)[None]).float())
    assert (kw["tv"], kw["l1"], kw["rate_floor"], kw["gt_times"]) == (0.0, 0.0, 0.5, 4.0)
    # rows that pull nothing up (max A^T h <= 0): lambda0 is 0, not negative, and the weights with it
    calls.clear()
    monkeypatch.setattr(Op, "adjoint", lambda self, r: torch.full((3, nr, 2), -7.0))
    out = LCT.lct_solve_capture({}, 0, nr, iterations=5, tv=0.25, l1=0.5)
    (kind, r, opkw, kw), = calls
    assert out["lambda0"] == 0.0 and (kw["tv"], kw["l1"]) == (0.0, 0.0)
    with pytest.raises(ValueError, match="loss"):
        LCT.lct_solve_capture({}, 0, nr, loss="huber")
    with pytest.raises(ValueError, match="rate_floor"):
        LCT.lct_solve_capture({}, 0, nr, loss="poisson", rate_floor=0.0)
