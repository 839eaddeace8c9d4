"""The LCT operator pair without a GPU: the four new entry points and their host-side validation, the float64
oracle's own identities (tests/lct_op_oracle.py: the adjoint identity, agreement with the light-cone transform's
adjoint), the float64 solvers on the point-scatterer scenes, the Python surface's refusals, the command line's new
flags and VoxelFitStep's new argument errors."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fk_oracle as FO
import lct_oracle as LO
import lct_op_oracle as OO
from nlosgr import lct as LCT

NEW = ("nlosgr_lct_load_volume", "nlosgr_lct_store_rows", "nlosgr_lct_load_rows", "nlosgr_lct_store_volume")


def test_library_carries_the_entry_points():
    from nlosgr import _lib
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.nlosgr_abi_version() == 13 and _lib.ABI_VERSION == 13
    import nlosgr
    for name in ("LctOperator", "lct_project", "lct_adjoint", "lct_solve", "lct_solve_capture", "lct_load_volume",
                 "lct_store_rows", "lct_load_rows", "lct_store_volume"):
        assert getattr(nlosgr, name) is getattr(LCT, name) and name in nlosgr.__all__, name


def test_entry_points_validate_on_the_host():
    """Every check runs before any launch and reports through nlosgr_last_error (no GPU; the fake non-null
    pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    err = lib.nlosgr_last_error

    def rows_pass(symbol):
        def call(data=fake, perm=None, H=4, W=6, nr=8, nv=8, sm=6, sn=1, r0=0.2, dr=0.01, power=-3, first=fake,
                 start=fake, weight=fake, nnz=15, out=other):
            return getattr(lib, symbol)(data, perm, H, W, nr, nv, sm, sn, r0, dr, power, first, start, weight, nnz,
                                        out, None)
        call.__name__ = symbol
        return call

    def volume_pass(symbol):
        def call(data=fake, H=4, W=6, nr=8, nv=8, first=fake, start=fake, weight=fake, nnz=15, out=other):
            return getattr(lib, symbol)(data, H, W, nr, nv, first, start, weight, nnz, out, None)
        call.__name__ = symbol
        return call

    load_rows, store_rows = rows_pass("nlosgr_lct_load_rows"), rows_pass("nlosgr_lct_store_rows")
    load_volume, store_volume = volume_pass("nlosgr_lct_load_volume"), volume_pass("nlosgr_lct_store_volume")
    for fn in (load_rows, store_rows, load_volume, store_volume):
        for bad in (dict(H=0), dict(W=-1), dict(H=1025), dict(W=1025), dict(nr=0), dict(nr=1025)):
            assert fn(**bad) == 1 and b"1..1024" in err(), (fn.__name__, bad)
        for bad in (dict(nv=0), dict(nv=-3), dict(nv=2049)):
            assert fn(**bad) == 1 and b"1..2048" in err(), (fn.__name__, bad)
        for nnz in (0, -1, 17):
            assert fn(nnz=nnz) == 1 and b"tables" in err(), (fn.__name__, nnz)
        for name in ("first", "start", "weight"):
            assert fn(**{name: None}) == 1 and b"table pointer" in err(), (fn.__name__, name)
        assert fn(data=None) == 1 and b"null" in err(), fn.__name__
        assert fn(out=None) == 1 and b"null" in err(), fn.__name__
    for fn in (load_rows, store_rows):
        for p in (-5, 5, 100):
            assert fn(power=p) == 1 and b"power must be in -4..4" in err(), (fn.__name__, p)
        for dr in (0.0, -0.01, float("inf"), float("nan")):
            assert fn(dr=dr) == 1 and b"dr" in err(), (fn.__name__, dr)
        for r0 in (-0.1, float("inf"), float("nan")):
            assert fn(r0=r0) == 1 and b"r0" in err(), (fn.__name__, r0)
        for sm, sn in ((-1, 1), (6, -1), (6, 2), (7, 1), (1, 6)):
            assert fn(sm=sm, sn=sn) == 1 and b"strides" in err(), (fn.__name__, sm, sn)
    # alignment: the work array of each pass; aliasing where the pass reads and writes arrays of one kind
    assert load_rows(out=ctypes.c_void_p(8200)) == 1 and b"16-byte aligned" in err()
    assert load_volume(out=ctypes.c_void_p(8196)) == 1 and b"8-byte aligned" in err()
    assert store_rows(data=ctypes.c_void_p(4100)) == 1 and b"8-byte aligned" in err()
    assert store_volume(data=ctypes.c_void_p(4100)) == 1 and b"8-byte aligned" in err()
    assert load_volume(out=fake) == 1 and b"alias" in err()
    assert store_rows(out=fake) == 1 and b"alias" in err()
    assert store_volume(out=fake) == 1 and b"alias" in err()
    # the old load keeps its own range
    assert lib.nlosgr_lct_load(fake, None, 4, 6, 8, 8, 6, 1, 0.2, 0.01, -1, fake, fake, fake, 15, other, None) == 1
    assert b"power must be in 0..4" in err()


def test_weights():
    w = OO.weights64(0.0, 0.5, 4, -2)
    assert np.array_equal(w, [0.0, 4.0, 1.0, 1.0 / 2.25])             # 0 where r <= 0, not inf
    assert np.array_equal(OO.weights64(0.5, 0.5, 3, 3), [0.125, 1.0, 3.375])
    assert np.array_equal(OO.weights64(0.0, 0.5, 3, 0), [1.0, 1.0, 1.0])


@pytest.mark.parametrize("name", list(FO.DENSE))
def test_oracle_adjoint_identity_and_agreement_with_the_transform(name):
    """<A v, h> = <v, A^T h> to 1e-12 for signed random v and h, at power -4, -3, 0, 4 and nv = nr, 2 nr - 3; and on
    non-negative rows A^T at power 4 is lct_oracle.reconstruct64(backprop=True) to 1e-14 of the maximum."""
    c = FO.DENSE[name]
    H, W, nr = c["H"], c["W"], c["nr"]
    r0, dr = FO.window(c)
    g = np.random.default_rng(17)
    for nv in (nr, 2 * nr - 3):
        for power in (-4, -3, 0, 4):
            op = OO.Operator64(H, W, c["sx"], c["sz"], r0, dr, nr, power, nv)
            v, h = g.standard_normal((W, nr, H)), g.standard_normal((H * W, nr))
            Av, Ath = op.forward(v), op.adjoint(h)
            assert Av.shape == (H * W, nr) and Ath.shape == (W, nr, H)
            gap = abs((Av * h).sum() - (v * Ath).sum()) / (np.sqrt((Av * Av).sum()) * np.sqrt((h * h).sum()))
            print(f"{name} nv {nv} power {power}: adjoint gap {gap:.2e}")
            assert gap <= 1e-12, (name, nv, power, gap)
        rows = np.abs(FO.dense_rows(c))
        got = OO.adjoint64(rows, H, W, c["sx"], c["sz"], r0, dr, power=4, nv=nv)
        want = LO.reconstruct64(rows, H, W, c["sx"], c["sz"], r0, dr, power=4, nv=nv, backprop=True)
        assert np.abs(got - want).max() <= 1e-14 * want.max(), (name, nv)
    # the row order: a shuffled perm and an x-major wall give the plain rows in permuted order
    op = OO.Operator64(H, W, c["sx"], c["sz"], r0, dr, nr, -3)
    v = g.standard_normal((W, nr, H))
    plain = op.forward(v)
    order = g.permutation(H * W)
    perm = np.argsort(order)
    shuffled = OO.project64(v, H, W, c["sx"], c["sz"], r0, dr, power=-3, perm=perm)
    assert np.array_equal(shuffled, plain[order])
    t = np.arange(H * W).reshape(H, W).T.reshape(-1)
    assert np.array_equal(OO.project64(v, H, W, c["sx"], c["sz"], r0, dr, power=-3, x_along="m"), plain[t])
    assert np.array_equal(OO.adjoint64(plain[order], H, W, c["sx"], c["sz"], r0, dr, power=-3, perm=perm),
                          op.adjoint(plain))


@pytest.mark.parametrize("index", range(len(LO.PEAKS)))
def test_oracle_solvers_on_a_point_scatterer(index):
    """30 projected-gradient steps in float64, power 0 against rows r^3: the objective never rises, the argmax is
    the scatterer's voxel, and FISTA ends with a lower 1/2 |A x - h|^2 than Landweber."""
    s = OO.peak_solution(index)
    c = s["case"]
    for key in ("landweber", "fista"):
        vol, obj = s[key]
        assert obj.shape == (30,) and (np.diff(obj) <= 0).all(), (key, obj)
        at = tuple(int(v) for v in np.unravel_index(int(vol.argmax()), vol.shape))
        assert at == c["voxel"], (key, at)
        assert (vol >= 0).all()
    lw, fi = s["final"]
    print(f"{LO.PEAKS[index][0]} nv {s['nv']}: norm {s['norm']:.6g}, Landweber {s['landweber'][1][-1]:.4g} -> "
          f"{lw:.4g}, FISTA {s['fista'][1][-1]:.4g} -> {fi:.4g}")
    assert fi < lw


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    rows = torch.zeros(24, 8)
    vol = torch.zeros(6, 8, 4)
    spec = torch.zeros(8, 12, 16, dtype=torch.complex64)
    res = LCT.lct_resampling(0.0, 0.01, 8)
    for call in (lambda: LCT.lct_load_rows(rows, 4, 6, 0.0, 0.01),
                 lambda: LCT.lct_load_volume(vol, res),
                 lambda: LCT.lct_store_rows(spec, res),
                 lambda: LCT.lct_store_volume(spec, res),
                 lambda: LCT.lct_project(vol, 4, 6, 0.1, 0.1, 0.0, 0.01),
                 lambda: LCT.lct_adjoint(rows, 4, 6, 0.1, 0.1, 0.0, 0.01),
                 lambda: LCT.LctOperator(4, 6, 0.1, 0.1, 0.0, 0.01, 8, device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for power in (-5, 5):
        with pytest.raises(ValueError, match="power"):
            LCT.LctOperator(4, 6, 0.1, 0.1, 0.0, 0.01, 8, power=power)
    with pytest.raises(ValueError, match="sx and sz"):
        LCT.LctOperator(4, 6, 0.0, 0.1, 0.0, 0.01, 8)
    with pytest.raises(ValueError, match="nv"):
        LCT.LctOperator(4, 6, 0.1, 0.1, 0.0, 0.01, 8, nv=2049)
    with pytest.raises(TypeError, match="LctOperator"):
        LCT.lct_solve(rows, None)


def test_command_line_arguments(capsys):
    base = ["cap.mat", "--start", "20", "--end", "100"]
    a = LCT.parse_args(base)
    assert (a.iterations, a.accelerate, a.falloff, a.power) == (0, True, 3.0, 4)
    a = LCT.parse_args(base + ["--iterations", "12"])
    assert (a.iterations, a.accelerate, a.falloff, a.power) == (12, True, 3.0, 0)
    a = LCT.parse_args(base + ["--iterations", "12", "--no-accelerate", "--falloff", "2.5", "--power", "-3"])
    assert (a.iterations, a.accelerate, a.falloff, a.power) == (12, False, 2.5, -3)
    for extra in (["--iterations", "-1"], ["--power", "-3"], ["--power", "-5", "--iterations", "3"]):
        with pytest.raises(SystemExit):
            LCT.parse_args(base + extra)
    capsys.readouterr()


def test_voxel_fit_step_operator_argument_errors():
    from nlosgr.voxel_fit import VoxelFitStep, parse_args
    from nlosgr.voxelize import VoxelGrid
    grid = VoxelGrid(tables=(torch.linspace(-0.2, 0.2, 6), torch.linspace(0.1, 0.5, 8), torch.linspace(-0.1, 0.1, 4)))
    rows, walls = torch.zeros(24, 8), torch.zeros(24, 3)
    model = SimpleNamespace()
    fake_op = SimpleNamespace(volume_shape=(6, 8, 4), rows_shape=(24, 8))
    with pytest.raises(TypeError, match="LctOperator"):
        VoxelFitStep(model, grid, (0, 0, 0), rows=rows, operator=fake_op)
    op = object.__new__(LCT.LctOperator)                               # no GPU here: the shape checks need no more
    op.H, op.W, op.nr, op.device = 4, 6, 8, torch.device("cpu")
    with pytest.raises(ValueError, match="operator= .* walls="):
        VoxelFitStep(model, grid, (0, 0, 0), rows=rows, operator=op, walls=walls)
    with pytest.raises(ValueError, match="operator= .* walls="):
        VoxelFitStep(model, grid, (0, 0, 0), rows=rows, operator=op, lasers=walls)
    with pytest.raises(ValueError, match="operator= belongs to rows="):
        VoxelFitStep(model, grid, (0, 0, 0), target_volume=torch.zeros(6, 8, 4), operator=op)
    op.nr = 9
    with pytest.raises(ValueError, match=r"\(6, 9, 4\)"):
        VoxelFitStep(model, grid, (0, 0, 0), rows=rows, operator=op)
    base = ["cap.mat", "--start", "0", "--end", "64", "--gaussians", "100", "--iterations", "5", "--out", "c.pt"]
    a = parse_args(base)
    assert "projector" not in vars(a) and "nv" not in vars(a)        # absent unless given: the exact projector
    a = parse_args(base + ["--projector", "lct", "--nv", "128", "--power", "-3"])
    assert a.projector == "lct" and a.nv == 128 and a.power == -3
    for bad in (["--power", "-3"], ["--nv", "64"], ["--projector", "fast"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
