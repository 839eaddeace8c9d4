"""Back-projection without a GPU: the identities of the float64 oracle (tests/backproject_oracle.py), the
fp32 emulation of the kernel's arithmetic against the bound the GPU tests use, the time filters' taps, the
host-side validation of nlosgr_backproject, the point-scatterer condition on the oracle, and the CLI's
argument parsing."""
import ctypes

import numpy as np
import pytest
import torch

import backproject_oracle as BO

S = BO.SCENE


def _scene(seed=0):
    walls = BO.relay_wall(*S["wall"])
    tabs = BO.linspace_tables(S["position"], S["size"], S["res"])
    r0, inv_dr = BO.scene_window()
    rows = np.random.default_rng(seed).standard_normal((walls.shape[0], S["nr"])).astype(np.float32)
    return rows, walls, tabs, r0, inv_dr


@pytest.mark.parametrize("power", [0, 1, 3])
def test_row_of_ones_counts_the_window(power):
    """h = 1: out = sum of d^p over the wall points whose u lies in [0, nr-1] (both bins inside), plus the ramp
    share (1 - |overshoot|) of the points on either end ramp."""
    _, walls, tabs, r0, inv_dr = _scene()
    nr = S["nr"]
    rows = np.ones((walls.shape[0], nr), dtype=np.float32)
    d = BO.distances64(walls, *tabs)
    out, _ = BO.backproject64(rows, walls, *tabs, r0, inv_dr, power, d=d)
    u = BO.bin_coordinate(d, r0, inv_dr)
    inside = (u >= 0) & (u <= nr - 1)
    ramp = np.where((u > -1) & (u < 0), u + 1, 0.0) + np.where((u > nr - 1) & (u < nr), nr - u, 0.0)
    want = (d ** power * (inside + ramp)).sum(axis=1).reshape(out.shape)
    assert inside.any() and (ramp > 0).any() and (~inside & (ramp == 0)).any()
    np.testing.assert_allclose(out, want, rtol=1e-12, atol=1e-12)
    full = inside.all(axis=1).reshape(out.shape)          # voxels that see every wall point inside the window
    assert full.any()
    np.testing.assert_allclose(out[full], (d ** power).sum(axis=1).reshape(out.shape)[full], rtol=1e-12)


def test_linearity_in_rows():
    """Small-integer rows, so 2 a - 3 b is exact in fp32 and the oracle sees exactly the combined input."""
    _, walls, tabs, r0, inv_dr = _scene()
    g = np.random.default_rng(1)
    a = g.integers(-50, 50, (walls.shape[0], S["nr"])).astype(np.float32)
    b = g.integers(-50, 50, a.shape).astype(np.float32)
    d = BO.distances64(walls, *tabs)
    f = lambda r: BO.backproject64(r, walls, *tabs, r0, inv_dr, 2, d=d, want_bound=False)[0]
    np.testing.assert_allclose(f(2 * a - 3 * b), 2 * f(a) - 3 * f(b), rtol=0, atol=1e-9)
    assert not f(np.zeros_like(a)).any()


def test_end_ramps_are_linear_and_continuous():
    """One wall point, voxels on a line away from it: s follows (1 + u) h[0] for -1 < u < 0 and (nr - u) h[nr-1]
    for nr-1 < u < nr, and is zero at and beyond u = -1 and u = nr."""
    nr, r0, inv_dr = 6, float(np.float32(0.5)), float(np.float32(8.0))
    walls = np.zeros((1, 3), dtype=np.float32)
    rows = np.array([[3.0, -1.0, 2.0, 0.5, 4.0, -2.0]], dtype=np.float32)
    ys = (0.5 + np.array([-2.5, -1.5, -1.0, -0.75, -0.25, 0.0, 5.0, 5.25, 5.5, 6.0, 7.0]) / 8.0).astype(np.float32)  # exact
    out, B = BO.backproject64(rows, walls, np.zeros(1, np.float32), ys, np.zeros(1, np.float32), r0, inv_dr, 0)
    want = [0.0, 0.0, 0.0, 0.25 * 3.0, 0.75 * 3.0, 3.0, -2.0, 0.75 * -2.0, 0.5 * -2.0, 0.0, 0.0]
    np.testing.assert_allclose(out.reshape(-1), want, rtol=0, atol=1e-15)
    assert B[0, 0, 0] == 0.0 and B[0, -1, 0] == 0.0 and B[0, 1, 0] > 0.0    # k = -3 / nr + 1: dark; k = -2: the ramp's foot


def test_emulated_fp32_kernel_is_within_the_bound():
    """The kernel's arithmetic restated in numpy fp32 stays far inside B (-s prints the worst share)."""
    rows, walls, tabs, r0, inv_dr = _scene()
    d = BO.distances64(walls, *tabs)
    for power in (0, 2, 4):
        out, B = BO.backproject64(rows, walls, *tabs, r0, inv_dr, power, d=d)
        e = BO.emulate32(rows, walls, *tabs, r0, inv_dr, power)
        share = float((np.abs(e.astype(np.float64) - out) / B).max())
        print(f"emulated fp32 power {power}: worst e/B {share:.4f}")
        assert share <= 1.0
        # a wrong bin (window shifted by one) or a wrong weight is far outside the bound
        wrong = BO.emulate32(np.roll(rows, 1, axis=1), walls, *tabs, r0, inv_dr, power)
        assert (np.abs(wrong.astype(np.float64) - out) > 100 * B).any()
        if power:
            wrongw = BO.emulate32(rows, walls, *tabs, r0, inv_dr, power - 1)
            assert (np.abs(wrongw.astype(np.float64) - out) > 100 * B).any()


def test_time_filter_taps():
    from nlosgr.backproject import time_filter
    from nlosgr.irf import convolve_time
    lap = time_filter("laplacian")
    assert lap.taps.tolist() == [-1.0, 2.0, -1.0] and lap.center == 1 and lap.background == 0.0
    for sigma in (0.8, 2.0, 5.0):
        log = time_filter("log", sigma_bins=sigma)
        w = log.taps.double().numpy()
        n = int(np.ceil(4 * sigma))
        assert len(log) == 2 * n + 3 and log.center == n + 1 and log.background == 0.0
        assert abs(w.sum()) <= len(w) * 2.0 ** -24 * np.abs(w).max()
        k = np.arange(-n, n + 1)
        g = np.exp(-0.5 * (k / sigma) ** 2)
        ref = np.convolve(g / g.sum(), [-1.0, 2.0, -1.0])             # the Laplacian of the Gaussian taps
        np.testing.assert_allclose(w, ref, rtol=0, atol=2.0 ** -24 * np.abs(ref).max())
        np.testing.assert_allclose(w, w[::-1], rtol=0, atol=1e-9)
    for filt in (lap, time_filter("log", sigma_bins=2.0)):
        L, c = len(filt), filt.center
        ramp = (0.25 * torch.arange(200, dtype=torch.float64) - 3.0)[None]
        y = convolve_time(ramp, filt)[0]
        assert y[L:-L].abs().max().item() <= 1e-5 and y[:c].abs().max().item() > 0.1   # interior 0, edges not
    # minus the second difference: a peak stays a positive peak
    y = convolve_time(torch.tensor([[0.0, 0.0, 1.0, 0.0, 0.0]], dtype=torch.float64), lap)[0]
    assert y.tolist() == [0.0, -1.0, 2.0, -1.0, 0.0]
    with pytest.raises(ValueError):
        time_filter("box")
    with pytest.raises(ValueError):
        time_filter("log", sigma_bins=0.0)
    with pytest.raises(ValueError):
        time_filter("log", sigma_bins=100.0)                           # more than 512 taps


def test_backproject_validates_on_the_host():
    """nlosgr_backproject checks its arguments before any launch and reports through nlosgr_last_error (no GPU;
    the fake non-null pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    V = lambda nx=8, ny=8, nz=8, p=fake: _lib.VoxelGrid(nx, ny, nz, p, p, p)
    O = lambda r0=0.2, inv=100.0, power=0, acc=0: _lib.BackprojectOpts(r0, inv, power, acc)

    def call(rows=fake, walls=fake, nwall=4, nr=16, v=None, o=None, out=fake, novg=False, noopt=False):
        v, o = v or V(), o or O()
        return lib.nlosgr_backproject(rows, walls, nwall, nr, None if novg else ctypes.byref(v),
                                      None if noopt else ctypes.byref(o), out, None)

    err = lib.nlosgr_last_error
    for bad in (dict(nx=0), dict(ny=0), dict(nz=-2), dict(nx=1025), dict(nz=4096)):
        assert call(v=V(**bad)) == 1 and b"1..1024" in err(), bad
    assert call(nr=0) == 1 and b"nr" in err()
    assert call(nwall=-1) == 1 and b"nwall" in err()
    for p in (-1, 5, 100):
        assert call(o=O(power=p)) == 1 and b"power" in err(), p
    for inv in (0.0, -3.0, float("inf"), float("nan")):
        assert call(o=O(inv=inv)) == 1 and b"inv_dr" in err(), inv
    assert call(o=O(r0=float("nan"))) == 1 and b"r0" in err()
    assert call(novg=True) == 1 and b"null" in err()
    assert call(noopt=True) == 1 and b"null" in err()
    assert call(v=V(p=None)) == 1 and b"table" in err()
    assert call(out=None) == 1 and b"output" in err()
    assert call(rows=None) == 1 and b"rows" in err()
    assert call(walls=None) == 1 and b"walls" in err()
    assert ctypes.sizeof(_lib.BackprojectOpts) == 16
    assert lib.nlosgr_abi_version() == 13


def test_point_scatterer_condition_on_the_oracle():
    """A scatterer at voxel (11, 5, 3) of the 17^3 grid, rows holding the linear splat at its time of flight:
    the back-projection peaks at that voxel and the runner-up is below half of it (0.32 measured)."""
    rows, walls, tabs, r0, inv_dr = BO.scatterer_scene()
    assert np.allclose(rows.sum(axis=1), 1.0, atol=1e-6)               # every wall point sees it inside the window
    out, _ = BO.backproject64(rows, walls, *tabs, r0, inv_dr, 0, want_bound=False)
    assert np.unravel_index(out.argmax(), out.shape) == S["voxel"]
    top = np.sort(out.reshape(-1))
    print(f"point scatterer: runner-up / peak {top[-2] / top[-1]:.3f}")
    assert top[-2] < 0.5 * top[-1]
    assert 0.5 * walls.shape[0] <= top[-1] <= walls.shape[0]           # every wall point adds (1-f)^2 + f^2 >= 1/2


def test_cli_argument_parsing():
    from nlosgr.backproject import parse_args
    a = parse_args(["cap.mat", "--resolution", "64", "--start", "100", "--end", "612", "--power", "2", "--filter",
                    "laplacian", "--sigma-bins", "3.5", "--out", "x.npz", "--mesh", "x.ply", "--level-frac", "0.3"])
    assert (a.capture, a.resolution, a.start, a.end, a.power, a.filter) == ("cap.mat", 64, 100, 612, 2, "laplacian")
    assert (a.sigma_bins, a.out, a.mesh, a.level_frac) == (3.5, "x.npz", "x.ply", 0.3)
    d = parse_args(["cap.mat", "--start", "0", "--end", "10"])
    assert (d.resolution, d.power, d.filter, d.sigma_bins, d.out, d.mesh) == (128, 0, "log", 2.0, "bp.npz", None)
    for bad in (["cap.mat", "--end", "10"], ["cap.mat", "--start", "5", "--end", "5"],
                ["cap.mat", "--start", "0", "--end", "9", "--power", "5"],
                ["cap.mat", "--start", "0", "--end", "9", "--filter", "box"], ["--start", "0", "--end", "9"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_python_surface_refuses_cpu_tensors():
    from nlosgr.backproject import backproject
    from nlosgr.voxelize import VoxelGrid
    grid = VoxelGrid((0.0, 0.5, 0.0), 0.5, 4)
    with pytest.raises(RuntimeError):
        backproject(torch.zeros(3, 8), torch.zeros(3, 3), grid, 0.0, 0.01)
