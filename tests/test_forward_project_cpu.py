"""Forward projection without a GPU: the float64 oracle (tests/forward_project_oracle.py) against the
back-projection's oracle (the adjoint identity), a hand-computed row, the closed-form shell integral of a
Gaussian, the host-side validation of nlosgr_forward_project, the Landweber iteration in float64 on the
point-scatterer scene, and the CLI's argument parsing."""
import ctypes

import numpy as np
import pytest
import torch

import backproject_oracle as BO
import forward_project_oracle as FO

S = BO.SCENE


def _tables(shape):
    nx, ny, nz = shape
    return (np.linspace(-0.3, 0.3, nx).astype(np.float32), np.linspace(0.0, 0.6, ny).astype(np.float32),
            np.linspace(-0.3, 0.3, nz).astype(np.float32))


@pytest.mark.parametrize("shape", [(9, 5, 13), (17, 17, 17)], ids=["9x5x13", "17^3"])
def test_adjoint_identity(shape):
    """<A v, h> = <v, A^T h> in float64 for the powers both operators take."""
    g = np.random.default_rng(3)
    tabs = _tables(shape)
    walls = np.array([[0.1, 0.0, -0.2], [-0.4, 0.0, 0.3], [0.0, 0.0, 0.0]], dtype=np.float32)
    nr, r0, inv_dr = 80, float(np.float32(0.2)), float(np.float32(1.0) / np.float32(0.01))
    v = g.standard_normal(shape).astype(np.float32)
    h = g.standard_normal((3, nr)).astype(np.float32)
    d = BO.distances64(walls, *tabs)
    for power in range(5):
        Av, _ = FO.forward64(v, walls, *tabs, r0, inv_dr, nr, power, d=d, want_bound=False)
        Ath, _ = BO.backproject64(h, walls, *tabs, r0, inv_dr, power, d=d, want_bound=False)
        lhs, rhs = float((Av * h).sum()), float((v.astype(np.float64) * Ath).sum())
        print(f"grid {shape} power {power}: <Av,h> {lhs:.12g} relative difference {abs(lhs - rhs) / abs(lhs):.2e}")
        assert Av.any() and abs(lhs - rhs) <= 1e-11 * abs(lhs)


@pytest.mark.parametrize("power", [-4, -1, 0, 3])
def test_one_voxel_volume_gives_its_scatterer_rows(power):
    walls = BO.relay_wall(4, 4)
    tabs = BO.linspace_tables(S["position"], S["size"], 9)
    r0, inv_dr = BO.scene_window()
    ix, iy, iz = 6, 2, 3
    vol = np.zeros((9, 9, 9), dtype=np.float32)
    vol[ix, iy, iz] = 2.5
    p = (tabs[0][ix], tabs[1][iy], tabs[2][iz])
    rows, B = FO.forward64(vol, walls, *tabs, r0, inv_dr, S["nr"], power)
    dist = np.sqrt(((walls.astype(np.float64) - np.array(p, dtype=np.float64)[None]) ** 2).sum(axis=1))
    want = 2.5 * dist[:, None] ** power * BO.scatterer_rows(walls, p, r0, inv_dr, S["nr"]).astype(np.float64)
    # scatterer_rows rounds its splat to fp32
    np.testing.assert_allclose(rows, want, rtol=2.0 ** -23, atol=0)
    assert (rows > 0).sum() == 2 * walls.shape[0] and (B[rows > 0] > 0).all()


def test_shell_integral_of_a_gaussian():
    """dV forward64(power -4) of an isotropic Gaussian (std 0.03, peak 1) on the 49^3 grid against
    dr / r^4 times the closed-form integral over the sphere of radius r: a condition on the oracle
    (-s prints the rel-L2; 33^3 gives 0.14)."""
    n, s, nr = 49, 0.03, 80
    tabs = BO.linspace_tables(S["position"], S["size"], n)
    r0, inv_dr = BO.scene_window()
    mu = np.array([tabs[0][24], tabs[1][24], tabs[2][24]], dtype=np.float64)
    X = BO.coords64(*tabs)
    vol = np.exp(-((X - mu[None]) ** 2).sum(axis=1) / (2 * s * s)).reshape(n, n, n)
    walls = np.array([[0.1, 0.0, -0.2], [-0.4, 0.0, 0.3], [0.0, 0.0, 0.0]], dtype=np.float32)
    rows, _ = FO.forward64(vol, walls, *tabs, r0, inv_dr, nr, -4, want_bound=False)
    dv = (S["size"] / (n - 1)) ** 3
    dr = 1.0 / inv_dr
    r = r0 + dr * np.arange(nr)
    D = np.sqrt(((walls.astype(np.float64) - mu[None]) ** 2).sum(axis=1))
    want = dr / r[None, :] ** 4 * FO.shell_integral(r[None, :], D[:, None], s)
    rel = float(np.linalg.norm(dv * rows - want) / np.linalg.norm(want))
    print(f"shell integral: rel-L2 {rel:.4f}")
    assert rel <= 0.01


def test_quantum_follows_the_header():
    r0, inv_dr = float(np.float32(0.3)), float(np.float32(1.0) / np.float32(0.015))
    # 16^3 voxels: S = 62 - 13; wmax = 1 (power 0) times the margin: ew = 1; vmax = 3 = 0.75 * 2^2: ev = 2
    assert FO.quantum(3.0, r0, inv_dr, 0, 40, 4096) == 2.0 ** (2 + 1 - 49)
    # power 2: R = 0.3 + 41 / inv_dr = 0.915, R^2 = 0.837 in [0.5, 1): ew = 0
    assert FO.quantum(3.0, r0, inv_dr, 2, 40, 4096) == 2.0 ** (2 + 0 - 49)
    # power -1: R = 0.3 - 1.5 * 0.015 = 0.2775, 1 / R = 3.6 = 0.9 * 2^2: ew = 2; one voxel: S = 61
    assert FO.quantum(0.5, r0, inv_dr, -1, 40, 1) == 2.0 ** (0 + 2 - 61)


def test_forward_project_validates_on_the_host():
    """Both entry points check their arguments before any launch and report through nlosgr_last_error (no GPU;
    the fake non-null pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    V = lambda nx=8, ny=8, nz=8, p=fake: _lib.VoxelGrid(nx, ny, nz, p, p, p)
    O = lambda r0=0.2, inv=100.0, power=0, acc=0, nsplit=0: _lib.ForwardProjectOpts(r0, inv, power, acc, nsplit)
    err = lib.nlosgr_last_error

    def call(vol=fake, walls=fake, nwall=4, nr=16, v=None, o=None, ws=fake, out=fake, novg=False, noopt=False):
        v, o = v or V(), o or O()
        return lib.nlosgr_forward_project(vol, walls, nwall, nr, None if novg else ctypes.byref(v),
                                          None if noopt else ctypes.byref(o), ws, out, None)

    def size(nwall=4, nr=16, v=None, o=None, novg=False, noopt=False):
        v, o = v or V(), o or O()
        return lib.nlosgr_forward_project_workspace_bytes(nwall, nr, None if novg else ctypes.byref(v),
                                                          None if noopt else ctypes.byref(o))

    def both(code, word, **kw):
        assert call(**kw) == code and word in err(), (kw, err())
        assert size(**kw) == 0 and word in err(), (kw, err())

    for bad in (dict(nx=0), dict(ny=0), dict(nz=-2), dict(nx=1025), dict(nz=4096)):
        both(1, b"1..1024", v=V(**bad))
    both(1, b"nr", nr=0)
    both(3, b"NLOSGR_IRF_MAX_NR", nr=8193)
    both(1, b"nwall", nwall=-1)
    for p in (-5, 5, 100):
        both(1, b"power", o=O(power=p))
    for inv in (0.0, -3.0, float("inf"), float("nan")):
        both(1, b"inv_dr", o=O(inv=inv))
    both(1, b"r0", o=O(r0=float("nan")))
    for r0 in (0.0, 0.019, -1.0):
        both(1, b"r0 * inv_dr", o=O(r0=r0, power=-1))
    both(1, b"nsplit", o=O(nsplit=-1))
    both(1, b"null", novg=True)
    both(1, b"null", noopt=True)
    both(1, b"table", v=V(p=None))
    assert call(vol=None) == 1 and b"vol" in err()
    assert call(walls=None) == 1 and b"walls" in err()
    assert call(ws=None) == 1 and b"workspace" in err()
    assert call(out=None) == 1 and b"output" in err()
    # valid sizes: the max|vol| word alone with one split, plus the int64 rows with more
    assert size(o=O(nsplit=1)) == 256
    assert size(nwall=4, nr=16, o=O(nsplit=2)) == 256 + 8 * 4 * 16
    assert size(nwall=0) == 256 and size(nr=8192) > 0
    assert size(o=O(r0=0.03, power=-4)) > 0 and size(o=O(power=4)) > 0
    # an empty wall is valid and launches nothing (no GPU here)
    assert call(nwall=0, walls=None, out=None) == 0
    assert ctypes.sizeof(_lib.ForwardProjectOpts) == 20
    assert lib.nlosgr_abi_version() == 13


@pytest.fixture(scope="module")
def landweber64():
    rows, walls, tabs, r0, inv_dr = BO.scatterer_scene()
    return FO.landweber64(rows, walls, tabs, r0, inv_dr)


def test_landweber_in_float64(landweber64):
    """30 projected-gradient steps on the point-scatterer scene (measured: objective 82.48 -> 43.60, runner-up /
    peak 0.201 against the back-projection's 0.315, largest eigenvalue 23920.565)."""
    x, obj, lam = landweber64
    top = np.sort(x.reshape(-1))
    print(f"landweber float64: objective {obj[0]:.2f} -> {obj[-1]:.2f}, runner-up / peak {top[-2] / top[-1]:.3f}, "
          f"eigenvalue {lam:.3f}")
    assert np.all(np.diff(obj) < 0)
    assert obj[-1] <= 0.6 * obj[0]
    assert int(x.argmax()) == 3267 and np.unravel_index(x.argmax(), x.shape) == S["voxel"]
    assert top[-2] <= 0.25 * top[-1]


def test_cli_argument_parsing():
    from nlosgr.forward_project import parse_args
    a = parse_args(["cap.mat", "--resolution", "32", "--start", "100", "--end", "612", "--power", "2", "--iterations",
                    "12", "--out", "x.npz", "--mesh", "x.ply", "--level-frac", "0.3"])
    assert (a.capture, a.resolution, a.start, a.end, a.power, a.iterations) == ("cap.mat", 32, 100, 612, 2, 12)
    assert (a.out, a.mesh, a.level_frac) == ("x.npz", "x.ply", 0.3)
    d = parse_args(["cap.mat", "--start", "0", "--end", "10"])
    assert (d.resolution, d.power, d.iterations, d.out, d.mesh, d.level_frac) == (64, 0, 30, "lw.npz", None, 0.5)
    for bad in (["cap.mat", "--end", "10"], ["cap.mat", "--start", "5", "--end", "5"],
                ["cap.mat", "--start", "0", "--end", "9", "--power", "5"],
                ["cap.mat", "--start", "0", "--end", "9", "--power", "-1"],
                ["cap.mat", "--start", "0", "--end", "9", "--iterations", "0"], ["--start", "0", "--end", "9"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_python_surface_refuses_cpu_tensors():
    from nlosgr.forward_project import forward_project, landweber, operator_norm
    from nlosgr.voxelize import VoxelGrid
    grid = VoxelGrid((0.0, 0.5, 0.0), 0.5, 4)
    with pytest.raises(RuntimeError):
        forward_project(torch.zeros(4, 4, 4), torch.zeros(3, 3), grid, 0.0, 0.01, 8)
    with pytest.raises(RuntimeError):
        landweber(torch.zeros(3, 8), torch.zeros(3, 3), grid, 0.0, 0.01)
    with pytest.raises(RuntimeError):
        operator_norm(torch.zeros(3, 3), grid, 0.0, 0.01, 8)
