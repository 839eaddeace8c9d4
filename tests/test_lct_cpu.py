"""The light-cone transform without a GPU: the float64 oracle (tests/lct_oracle.py) puts point scatterers at their
voxel, the identities of the resampling operator and its run tables, the host-side validation of the four new entry
points, the Python surface's refusals, the command line's arguments, and init.sample_from_volume on CPU tensors."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fk_oracle as FO
import lct_oracle as LO
from nlosgr import lct as LCT


def test_library_carries_the_entry_points():
    from nlosgr import _lib
    lib = _lib.load()
    for name in ("nlosgr_lct_load", "nlosgr_lct_kernel", "nlosgr_lct_filter", "nlosgr_lct_store"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.nlosgr_abi_version() == 13
    import nlosgr
    assert nlosgr.lct_reconstruct is LCT.lct_reconstruct and nlosgr.lct_capture is LCT.lct_capture


@pytest.mark.parametrize("name,nv,voxel", LO.PEAKS)
def test_oracle_puts_a_point_scatterer_at_its_voxel(name, nv, voxel):
    """The definition itself, in float64: the volume of one point scatterer peaks exactly at its voxel, at the
    default snr and at a sharp one, with sx != sz, and with a window that starts at bin 20 or 35.  On the r0 = 35 dr
    lattice the near voxel (6, 8, 9) needs nv = 128: at nv = 64 a near cell is two bins deep and the peak sits one
    bin early, which the last assertion pins."""
    c = LO.peak_case(name, voxel)
    rows, xs, zs, r0, dr = FO.scatterer_scene(c)
    for snr in (0.8, 100.0):
        vol = LO.reconstruct64(rows, c["H"], c["W"], c["sx"], c["sz"], r0, dr, snr=snr, nv=nv)
        assert vol.shape == (c["W"], c["nr"], c["H"]) and (vol >= 0).all()
        at, ratio = FO.peak(vol + 1e-300)
        print(f"{name} nv {nv} snr {snr:g}: argmax {at}, peak / median {ratio:.3g}")
        assert at == c["voxel"]
    if name == "16x16x64_r35" and nv == 128:
        early = LO.reconstruct64(rows, c["H"], c["W"], c["sx"], c["sz"], r0, dr, nv=64)
        assert FO.peak(early)[0] == (6, 7, 9)


RESAMPLINGS = [(0.0, 0.02, 64, None), (0.0, 0.02, 48, 96), (0.09, 0.03, 17, 23), (0.09, 0.03, 17, 34),
               (0.7, 0.02, 64, 128), (0.0, 0.04, 16, 1), (0.3, 0.01, 1, 5), (0.005, 0.02, 9, 2048)]


@pytest.mark.parametrize("r0,dr,nr,nv", RESAMPLINGS)
def test_resampling_identities_and_tables(r0, dr, nr, nv):
    res = LCT.lct_resampling(r0, dr, nr, nv)
    nv = nr if nv is None else nv
    e, t, dv = LO.edges64(r0, dr, nr, nv)
    assert (res.nr, res.nv) == (nr, nv) and res.dv == dv and dv > 0
    assert t[0] == e[0] == max(FO.f32(r0) - FO.f32(dr) / 2, 0.0) and t[nv] == e[nr]
    R64, _ = LO.resampling64(r0, dr, nr, nv)
    R = res.dense().numpy()
    # the tables hold the float64 operator rounded to fp32, nothing else
    assert np.array_equal(R, R64.astype(np.float32).astype(np.float64))
    assert np.array_equal(R != 0, R64 > 0)
    # row i sums to 1 / (the cell's mean radius); the dv-weighted mass of bin j is the bin's width
    mean = (t[:-1] + t[1:]) / 2
    assert np.allclose(R64.sum(axis=1), 1.0 / mean, rtol=1e-9, atol=0)
    assert np.allclose(R.sum(axis=1), 1.0 / mean, rtol=2.0 ** -23, atol=0)
    width = (t[1:] - t[:-1]) * mean                                  # = dv / 2
    assert np.allclose(width, dv / 2, rtol=1e-9, atol=0)
    assert np.allclose((R64 * width[:, None]).sum(axis=0), e[1:] - e[:-1], rtol=1e-9, atol=0)
    assert np.allclose((R * width[:, None]).sum(axis=0), e[1:] - e[:-1], rtol=2.0 ** -23, atol=0)
    # runs: contiguous, monotone, nnz <= nv + nr; R^T's tables hold the same entries
    nnz = res.nnz
    assert 1 <= nnz <= nv + nr and nnz == int((R64 > 0).sum())
    for first, start, weight, M in ((res.first, res.start, res.weight, R), (res.first_t, res.start_t, res.weight_t, R.T)):
        assert first.dtype == start.dtype == torch.int32 and weight.dtype == torch.float32
        assert start.shape == (M.shape[0] + 1,) and first.shape == (M.shape[0],) and weight.shape == (nnz,)
        first, start, weight = first.numpy(), start.numpy(), weight.numpy()
        assert start[0] == 0 and start[-1] == nnz and (np.diff(start) >= 1).all() and (np.diff(first) >= 0).all()
        for i in range(M.shape[0]):
            n = start[i + 1] - start[i]
            run = M[i, first[i]:first[i] + n]
            assert (run > 0).all() and np.array_equal(run, weight[start[i]:start[i + 1]].astype(np.float64))
            assert M[i].sum() == run.sum()                          # nothing outside the run
    assert np.array_equal(np.sort(res.weight.numpy()), np.sort(res.weight_t.numpy()))


def test_resampling_refuses_bad_windows():
    for bad in (dict(nr=0), dict(nr=1025), dict(nv=0), dict(nv=2049), dict(dr=0.0), dict(dr=-1.0), dict(r0=-0.1),
                dict(dr=float("nan")), dict(r0=float("inf"))):
        kw = dict(r0=0.1, dr=0.01, nr=16, nv=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            LCT.lct_resampling(**kw)


def test_oracle_stages_compose():
    c = FO.DENSE["5x7x17_r3"]
    rows = FO.dense_rows(c)
    r0, dr = FO.window(c)
    H, W, nr, nv = c["H"], c["W"], c["nr"], 23
    R, dv = LO.resampling64(r0, dr, nr, nv)
    pad = LO.load64(rows, H, W, r0, dr, R)
    assert pad.shape == (2 * H, 2 * W, 2 * nv) and not pad[H:].any() and not pad[:, W:].any() and not pad[:, :, nv:].any()
    K, scale = LO.kernel64(H, W, nv, c["sx"], c["sz"], dv)
    assert abs((K * K).sum() - 1.0) < 1e-12 and (K >= 0).all() and not K[:, :, nv:].any()
    assert ((K != 0).sum(axis=2) <= 2).all() and K[0, 0, 0] == scale and (K[0, 0, 1:] == 0).all()
    assert abs(LCT.lct_scale(H, W, nv, c["sx"], c["sz"], dv) / scale - 1.0) <= 1e-14     # (the sums' order differs)
    # the kernel is even in both lattice offsets
    assert np.array_equal(K[1:H], K[:H:-1]) and np.array_equal(K[:, 1:W], K[:, :W:-1])
    G = LO.inverse64(np.fft.fftn(K), 0.8)
    S = np.fft.fftn(pad)
    vol = LO.store64(np.fft.ifftn(S * G), H, W, R)
    assert np.array_equal(vol, LO.reconstruct64(rows, H, W, c["sx"], c["sz"], r0, dr, nv=nv))
    assert vol.shape == (W, nr, H) and (vol >= 0).all() and (vol == 0).any() and (vol > 0).any()
    Gb = LO.inverse64(np.fft.fftn(K), 0.8, backprop=True)
    assert np.array_equal(Gb, np.conj(np.fft.fftn(K)))


def test_entry_points_validate_on_the_host():
    """Every check runs before any launch and reports through nlosgr_last_error (no GPU; the fake non-null
    pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    err = lib.nlosgr_last_error

    def load(rows=fake, perm=None, H=4, W=6, nr=8, nv=8, sm=6, sn=1, r0=0.2, dr=0.01, power=4, first=fake, start=fake,
             weight=fake, nnz=15, pad=fake):
        return lib.nlosgr_lct_load(rows, perm, H, W, nr, nv, sm, sn, r0, dr, power, first, start, weight, nnz, pad, None)

    def kernel(H=4, W=6, nv=8, sx=0.1, sz=0.1, dv=0.001, scale=0.1, K=fake):
        return lib.nlosgr_lct_kernel(H, W, nv, sx, sz, dv, scale, K, None)

    def filt(kf=fake, spec=other, H=4, W=6, nv=8, snr=0.8, mode=0, out=other):
        return lib.nlosgr_lct_filter(kf, spec, H, W, nv, snr, mode, out, None)

    def store(field=fake, H=4, W=6, nr=8, nv=8, first=fake, start=fake, weight=fake, nnz=15, vol=other):
        return lib.nlosgr_lct_store(field, H, W, nr, nv, first, start, weight, nnz, vol, None)

    for fn in (load, kernel, filt, store):
        for bad in (dict(H=0), dict(W=-1), dict(H=1025), dict(W=1025)):
            assert fn(**bad) == 1 and b"1..1024" in err(), (fn.__name__, bad)
        for bad in (dict(nv=0), dict(nv=-3), dict(nv=2049)):
            assert fn(**bad) == 1 and b"1..2048" in err(), (fn.__name__, bad)
    for fn in (load, store):
        for bad in (dict(nr=0), dict(nr=1025)):
            assert fn(**bad) == 1 and b"1..1024" in err(), (fn.__name__, bad)
        for nnz in (0, -1, 17):
            assert fn(nnz=nnz) == 1 and b"tables" in err(), (fn.__name__, nnz)
        for name in ("first", "start", "weight"):
            assert fn(**{name: None}) == 1 and b"table pointer" in err(), (fn.__name__, name)
    for dr in (0.0, -0.01, float("inf"), float("nan")):
        assert load(dr=dr) == 1 and b"dr" in err(), dr
    for r0 in (-0.1, float("inf"), float("nan")):
        assert load(r0=r0) == 1 and b"r0" in err(), r0
    for p in (-1, 5, 100):
        assert load(power=p) == 1 and b"power" in err(), p
    for sm, sn in ((-1, 1), (6, -1), (6, 2), (7, 1), (1, 6)):
        assert load(sm=sm, sn=sn) == 1 and b"strides" in err(), (sm, sn)
    assert load(rows=None) == 1 and b"rows" in err()
    assert load(pad=None) == 1 and b"padded" in err()
    assert load(pad=ctypes.c_void_p(4104)) == 1 and b"aligned" in err()
    for bad in (dict(sx=0.0), dict(sz=-1.0), dict(sx=float("nan")), dict(sz=float("inf"))):
        assert kernel(**bad) == 1 and b"sx and sz" in err(), bad
    for dv in (0.0, -1e-3, float("nan"), float("inf")):
        assert kernel(dv=dv) == 1 and b"dv" in err(), dv
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        assert kernel(scale=scale) == 1 and b"scale" in err(), scale
    assert kernel(K=None) == 1 and b"kernel array" in err()
    assert kernel(K=ctypes.c_void_p(4104)) == 1 and b"aligned" in err()
    for snr in (0.0, -1.0, float("nan"), float("inf")):
        assert filt(snr=snr) == 1 and b"snr" in err(), snr
    for mode in (-1, 3):
        assert filt(mode=mode) == 1 and b"mode" in err(), mode
    assert filt(kf=None) == 1 and b"kernel spectrum" in err()
    assert filt(out=None) == 1 and b"output" in err()
    assert filt(spec=None, mode=2) == 1 and b"given inverse" in err()
    for name in ("kf", "spec", "out"):
        assert filt(**{name: ctypes.c_void_p(4104)}) == 1 and b"aligned" in err(), name
    assert store(field=None) == 1 and b"field" in err()
    assert store(vol=None) == 1 and b"volume" in err()
    assert store(field=ctypes.c_void_p(4100)) == 1 and b"aligned" in err()
    assert store(vol=fake) == 1 and b"alias" in err()


def test_python_surface_refuses_cpu_tensors_and_bad_arguments():
    rows = torch.zeros(24, 8)
    spec = torch.zeros(8, 12, 16, dtype=torch.complex64)
    res = LCT.lct_resampling(0.0, 0.01, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LCT.lct_reconstruct(rows, 4, 6, 0.1, 0.1, 0.0, 0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LCT.lct_load(rows, 4, 6, 0.0, 0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LCT.lct_kernel(4, 6, 8, 0.1, 0.1, res.dv, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LCT.lct_filter(spec, kf=spec)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LCT.lct_store(spec, res)
    with pytest.raises(ValueError):
        LCT.lct_filter(spec)                                          # neither kf= nor inverse=
    with pytest.raises(ValueError):
        LCT.lct_filter(spec, kf=spec, inverse=spec)
    with pytest.raises(ValueError):
        LCT.lct_reconstruct(rows, 4, 6, 0.0, 0.1, 0.0, 0.01)
    for snr in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="snr"):
            LCT.lct_reconstruct(rows, 4, 6, 0.1, 0.1, 0.0, 0.01, snr=snr)
        with pytest.raises(ValueError, match="snr"):
            LCT.lct_inverse(4, 6, 8, 0.1, 0.1, res.dv, snr)
    for nv in (0, 2049):
        with pytest.raises(ValueError, match="nv"):
            LCT.lct_kernel(4, 6, nv, 0.1, 0.1, res.dv)


def test_command_line_arguments(capsys):
    a = LCT.parse_args(["cap.mat", "--start", "20", "--end", "100"])
    assert (a.power, a.snr, a.nv, a.backprop, a.out, a.mesh, a.level_frac) == (4, 0.8, None, False, "lct.npz", None, 0.5)
    a = LCT.parse_args(["cap.mat", "--start", "0", "--end", "64", "--power", "2", "--snr", "10", "--nv", "128",
                        "--backprop", "--mesh", "m.ply"])
    assert (a.power, a.snr, a.nv, a.backprop, a.mesh) == (2, 10.0, 128, True, "m.ply")
    for end in ("20", "19"):
        with pytest.raises(SystemExit):
            LCT.parse_args(["cap.mat", "--start", "20", "--end", end])
        assert "--end must be greater than --start" in capsys.readouterr().err
    for extra in (["--power", "5"], ["--snr", "0"], ["--nv", "0"], ["--nv", "2049"]):
        with pytest.raises(SystemExit):
            LCT.parse_args(["cap.mat", "--start", "20", "--end", "100"] + extra)


def test_sample_from_volume_draws_by_hand_on_cpu_tensors():
    from nlosgr.init import sample_from_volume
    from nlosgr.voxelize import VoxelGrid
    xs, ys, zs = torch.linspace(-0.4, 0.4, 9), torch.linspace(0.5, 0.9, 5), torch.linspace(-0.3, 0.3, 7)
    grid = VoxelGrid(tables=(xs, ys, zs))
    g = torch.Generator().manual_seed(11)
    vol = torch.rand((9, 5, 7), generator=g)
    vol[2, 1, 3] = -5.0                                               # clamped at 0: never drawn
    dk = {"pmin": torch.tensor([-0.4, 0.4, -0.3, 0.0]), "pmax": torch.tensor([0.4, 1.0, 0.3, 0.0])}
    args = SimpleNamespace(init_gaussian_num=300)
    for gamma in (1.0, 2.0):
        np.random.seed(5)
        torch.manual_seed(5)
        pts, rho = sample_from_volume(args, dk, vol, grid, margin=0.1, rho_scale=0.2, gamma=gamma)
        np.random.seed(5)
        torch.manual_seed(5)
        wrho = np.random.rand(300, 1) * 0.2
        lo = dk["pmin"][:3] + (dk["pmin"][:3] * 0.1).abs()
        hi = dk["pmax"][:3] - (dk["pmax"][:3] * 0.1).abs()
        inside = (((xs >= lo[0]) & (xs <= hi[0]))[:, None, None] & ((ys >= lo[1]) & (ys <= hi[1]))[None, :, None]
                  & ((zs >= lo[2]) & (zs <= hi[2]))[None, None, :])
        assert not inside.all() and inside.any()
        w = torch.where(inside, vol, torch.zeros_like(vol)).clamp_min(0).reshape(-1).double() ** gamma
        idx = torch.multinomial(w / w.sum(), 300, replacement=True)
        base = torch.stack((xs[idx // 35], ys[(idx // 7) % 5], zs[idx % 7]), dim=1)
        half = torch.stack([(t[-1] - t[0]) / (t.numel() - 1) for t in (xs, ys, zs)]) / 2
        want = base + (torch.rand_like(base) - 0.5) * 2 * half[None]
        assert torch.equal(pts, want) and np.array_equal(rho, wrho) and pts.shape == (300, 3) and rho.shape == (300, 1)
        assert not (idx == (2 * 5 + 1) * 7 + 3).any()
    with pytest.raises(RuntimeError, match="nothing to sample"):
        sample_from_volume(args, dk, torch.zeros(9, 5, 7), grid)
    with pytest.raises(RuntimeError, match="nothing to sample"):
        sample_from_volume(args, dk, torch.full((9, 5, 7), float("nan")), grid)
    with pytest.raises(ValueError):
        sample_from_volume(args, dk, torch.ones(9, 5, 6), grid)
