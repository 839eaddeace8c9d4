"""f-k migration without a GPU: the float64 oracle (tests/fk_oracle.py) puts point scatterers at their voxel, the
wall lattice of a capture (shuffled, unshuffled, transposed; an irregular or tilted wall raises), the tables of
fk_grid, and the host-side validation of the three new entry points."""
import ctypes

import numpy as np
import pytest
import torch

import fk_oracle as FO
from nlosgr import fk as FK


def test_library_carries_the_entry_points():
    from nlosgr import _lib
    lib = _lib.load()
    for name in ("nlosgr_fk_load", "nlosgr_fk_stolt", "nlosgr_fk_store"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.nlosgr_abi_version() == 13


@pytest.mark.parametrize("name", list(FO.SCATTERERS))
def test_oracle_puts_a_point_scatterer_at_its_voxel(name):
    """The definition itself, in float64: the volume of one point scatterer peaks exactly at its voxel, also with
    sx != sz and with a window that starts at bin 20 or 35 (the Stolt phase factor).  The peak stands 4e4 to 7e5
    times above the median, so the fp32 kernels, held to 2e-5 of the maximum, keep the argmax."""
    c = FO.SCATTERERS[name]
    rows, xs, zs, r0, dr = FO.scatterer_scene(c)
    assert rows.shape == (c["H"] * c["W"], c["nr"]) and (rows.sum(axis=1) > 0).mean() > 0.5
    vol = FO.migrate64(rows, c["H"], c["W"], c["sx"], c["sz"], r0, dr)
    assert vol.shape == (c["W"], c["nr"], c["H"])
    at, ratio = FO.peak(vol)
    print(f"{name}: argmax {at}, peak / median {ratio:.3g}")
    assert at == c["voxel"] and ratio >= 1e4


def test_oracle_stages_compose_and_mask():
    c = FO.DENSE["5x7x17_r3"]
    rows = FO.dense_rows(c)
    r0, dr = FO.window(c)
    H, W, nr = c["H"], c["W"], c["nr"]
    assert (rows < 0).any()
    pad = FO.load64(rows, H, W, r0, dr, power=4, amplitude=True)
    assert pad.shape == (2 * H, 2 * W, 2 * nr) and not pad[H:].any() and not pad[:, W:].any() and not pad[:, :, nr:].any()
    want = np.sqrt(max(float(rows[2 * W + 3, 5]), 0.0) * (r0 + 5 * dr) ** 4)
    assert pad[2, 3, 5] == want and (pad.real >= 0).all() and (pad[:H, :W, :nr].real == 0).any()
    V = FO.stolt64(np.fft.fftn(pad), c["sx"], c["sz"], r0, dr)
    assert not V[:, :, 0].any() and not V[:, :, nr - 1:].any() and V[:, :, 1:nr - 1].any()
    # the column b = c = 0 maps every bin to itself with weight 1 and no phase
    S = np.fft.fftn(pad)
    assert np.allclose(V[0, 0, 1:nr - 1], S[0, 0, 1:nr - 1], rtol=1e-12, atol=0)
    vol = FO.store64(np.fft.ifftn(V), H, W, nr)
    assert np.array_equal(vol, FO.migrate64(rows, H, W, c["sx"], c["sz"], r0, dr))
    # a permuted capture with its perm, and the transposed wall order, are the same lattice
    g = np.random.default_rng(1)
    order = g.permutation(H * W)                       # shuffled row u holds lattice point order[u]
    perm = np.argsort(order)
    assert np.array_equal(FO.load64(rows[order], H, W, r0, dr, perm=perm), pad)
    t = np.arange(H * W).reshape(H, W).T.reshape(-1)   # row n H + m holds lattice point m W + n
    assert np.array_equal(FO.load64(rows[t], H, W, r0, dr, x_along="m"), pad)


def _capture(H, W, shuffle=False, transpose=False, device="cpu"):
    """data_kwargs of an H x W relay wall as make_data_kwargs builds them (the keys wall_lattice reads)."""
    from nlosgr.geometry import relay_wall_grid
    walls = relay_wall_grid(H, W, extent=1.0)                     # [H W, 3], m W + n
    M, N = H, W
    if transpose:                                                 # x runs along the first wall index
        walls = walls.reshape(H, W, 3).transpose(0, 1).reshape(-1, 3)
        M, N = W, H
    pos = walls.t().contiguous()
    index = torch.arange(M * N, dtype=torch.float)
    if shuffle:
        order = torch.randperm(M * N, generator=torch.Generator().manual_seed(3))
        pos, index = pos[:, order], index[order]
    return {"nlos_data": torch.zeros(4, M, N), "camera_grid_positions": pos.to(device), "index": index.to(device)}


def test_wall_lattice_of_a_relay_wall():
    from nlosgr.geometry import relay_wall_grid
    H, W = 6, 10
    walls = relay_wall_grid(H, W).numpy()
    for shuffle in (False, True):
        dk = _capture(H, W, shuffle=shuffle)
        h, w, xs, zs, y0, perm, x_along = FK.wall_lattice(dk)
        assert (h, w, x_along, y0) == (H, W, "n", 0.0)
        assert xs.dtype == zs.dtype == torch.float32 and perm.dtype == torch.int32
        assert np.array_equal(xs.numpy(), walls[:W, 0]) and np.array_equal(zs.numpy(), walls[::W, 2])
        # column perm[v] of the capture is lattice point v
        assert torch.equal(dk["camera_grid_positions"][:, perm.long()], torch.from_numpy(walls).t())
        assert torch.equal(dk["index"][perm.long()], torch.arange(H * W, dtype=torch.float))
        assert abs(FK.lattice_spacing(xs) - 0.1) < 1e-7 and abs(FK.lattice_spacing(zs) - 1 / 6) < 1e-7
    for shuffle in (False, True):
        dk = _capture(H, W, shuffle=shuffle, transpose=True)
        h, w, xs, zs, y0, perm, x_along = FK.wall_lattice(dk)
        assert (h, w, x_along) == (H, W, "m")
        assert np.array_equal(xs.numpy(), walls[:W, 0]) and np.array_equal(zs.numpy(), walls[::W, 2])
        # lattice point (m, n) is unshuffled wall point n H + m
        v = (np.arange(W)[None, :] * H + np.arange(H)[:, None]).reshape(-1)
        got = dk["camera_grid_positions"][:, perm.long()][:, v]
        assert torch.equal(got, torch.from_numpy(walls).t())
    h, w, xs, zs, *_ , x_along = FK.wall_lattice(_capture(1, 9))
    assert (h, w, x_along) == (1, 9, "n") and FK.lattice_spacing(zs, FK.lattice_spacing(xs)) == FK.lattice_spacing(xs)


def test_wall_lattice_refuses_what_is_not_a_lattice():
    H, W = 6, 10
    base = _capture(H, W)
    sx = 0.1

    def moved(fn):
        dk = dict(base)
        pos = base["camera_grid_positions"].clone()
        fn(pos)
        dk["camera_grid_positions"] = pos
        return dk

    def bump(pos):
        pos[0, 23] += 2e-4 * sx                               # one point 2e-4 of the spacing off

    def tilt(pos):
        pos[1] += 0.01 * pos[0]                               # the plane leans: y = 0.01 x

    def shear(pos):
        pos[2] += 0.02 * pos[0]                               # rows not parallel to x

    def stretch(pos):
        pos[0] = pos[0] * pos[0].abs()                        # non-uniform spacing

    def flip(pos):
        pos[0] = -pos[0]                                      # x decreases along its axis

    for fn in (bump, tilt, shear, stretch, flip):
        with pytest.raises(ValueError):
            FK.wall_lattice(moved(fn))
    ok = moved(lambda pos: pos[0, 23].add_(2e-5 * sx))       # within 1e-4 of the spacing
    assert FK.wall_lattice(ok)[:2] == (H, W)
    with pytest.raises(ValueError):
        FK.wall_lattice(_capture(1, 1))
    dk = dict(base)
    dk["index"] = torch.zeros(H * W)
    with pytest.raises(ValueError):
        FK.wall_lattice(dk)


def test_fk_grid_tables():
    xs = torch.linspace(-0.45, 0.45, 10)
    zs = torch.linspace(-0.4, 0.4, 6)
    r0, dr = 20 * 0.01, 0.01
    grid = FK.fk_grid(xs, zs, 0.25, r0, dr, 48)
    assert grid.shape == (10, 48, 6)
    assert torch.equal(grid.xs, xs) and torch.equal(grid.zs, zs)
    want = (0.25 + r0 + dr * np.arange(48)).astype(np.float32)
    assert np.array_equal(grid.ys.numpy(), want) and grid.ys.dtype == torch.float32
    sub = grid.slice((2, 5), (10, 20), None)
    assert sub.shape == (3, 10, 6) and torch.equal(sub.ys, grid.ys[10:20])
    assert FK.fk_grid(xs, zs, 0.0, 0.0, dr, 1024).shape == (10, 1024, 6)
    with pytest.raises(ValueError):
        FK.fk_grid(xs, zs, 0.0, 0.0, dr, 1025)
    with pytest.raises(ValueError):
        FK.fk_grid(torch.zeros(1025), zs, 0.0, 0.0, dr, 8)


def test_entry_points_validate_on_the_host():
    """Every check runs before any launch and reports through nlosgr_last_error (no GPU; the fake non-null
    pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    err = lib.nlosgr_last_error

    def load(rows=fake, perm=None, H=4, W=6, nr=8, sm=6, sn=1, r0=0.2, dr=0.01, power=4, amp=1, pad=fake):
        return lib.nlosgr_fk_load(rows, perm, H, W, nr, sm, sn, r0, dr, power, amp, pad, None)

    def stolt(spec=fake, H=4, W=6, nr=8, sx=0.1, sz=0.1, r0=0.2, dr=0.01, out=ctypes.c_void_p(8192)):
        return lib.nlosgr_fk_stolt(spec, H, W, nr, sx, sz, r0, dr, out, None)

    def store(field=fake, H=4, W=6, nr=8, vol=fake):
        return lib.nlosgr_fk_store(field, H, W, nr, vol, None)

    for fn in (load, stolt, store):
        for bad in (dict(H=0), dict(W=-1), dict(nr=0), dict(H=1025), dict(W=1025), dict(nr=1025)):
            assert fn(**bad) == 1 and b"1..1024" in err(), (fn.__name__, bad)
    for fn in (load, stolt):
        for dr in (0.0, -0.01, float("inf"), float("nan")):
            assert fn(dr=dr) == 1 and b"dr" in err(), (fn.__name__, dr)
        for r0 in (-0.1, float("inf"), float("nan")):
            assert fn(r0=r0) == 1 and b"r0" in err(), (fn.__name__, r0)
    for p in (-1, 5, 100):
        assert load(power=p) == 1 and b"power" in err(), p
    for sm, sn in ((-1, 1), (6, -1), (6, 2), (7, 1), (1, 6)):     # the last lattice point would leave [0, H W)
        assert load(sm=sm, sn=sn) == 1 and b"strides" in err(), (sm, sn)
    assert load(rows=None) == 1 and b"rows" in err()
    assert load(pad=None) == 1 and b"padded" in err()
    assert load(pad=ctypes.c_void_p(4104)) == 1 and b"aligned" in err()
    for bad in (dict(sx=0.0), dict(sz=-1.0), dict(sx=float("nan")), dict(sz=float("inf"))):
        assert stolt(**bad) == 1 and b"sx and sz" in err(), bad
    assert stolt(spec=None) == 1 and b"spectrum" in err()
    assert stolt(out=None) == 1 and b"migrated" in err()
    assert stolt(out=fake) == 1 and b"alias" in err()
    assert stolt(spec=ctypes.c_void_p(4100)) == 1 and b"aligned" in err()
    assert store(field=None) == 1 and b"field" in err()
    assert store(vol=None) == 1 and b"volume" in err()
    assert store(field=ctypes.c_void_p(4100)) == 1 and b"aligned" in err()


def test_python_surface_refuses_cpu_tensors_and_bad_shapes():
    rows = torch.zeros(24, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FK.fk_migrate(rows, 4, 6, 0.1, 0.1, 0.0, 0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FK.fk_stolt(torch.zeros(8, 12, 16, dtype=torch.complex64), 0.1, 0.1, 0.0, 0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FK.fk_store(torch.zeros(8, 12, 16, dtype=torch.complex64))
    with pytest.raises(ValueError):
        FK.fk_migrate(rows, 4, 6, 0.0, 0.1, 0.0, 0.01)


def test_command_line_arguments(capsys):
    a = FK.parse_args(["cap.mat", "--start", "20", "--end", "100"])
    assert (a.power, a.no_amplitude, a.out, a.mesh, a.level_frac) == (4, False, "fk.npz", None, 0.5)
    a = FK.parse_args(["cap.mat", "--start", "0", "--end", "64", "--power", "2", "--no-amplitude", "--mesh", "m.ply"])
    assert (a.power, a.no_amplitude, a.mesh) == (2, True, "m.ply")
    for end in ("20", "19"):
        with pytest.raises(SystemExit):
            FK.parse_args(["cap.mat", "--start", "20", "--end", end])
        assert "--end must be greater than --start" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        FK.parse_args(["cap.mat", "--start", "20", "--end", "100", "--power", "5"])
