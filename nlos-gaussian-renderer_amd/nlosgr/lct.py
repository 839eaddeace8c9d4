"""The light-cone transform of a confocal capture (LCT; O'Toole, Lindell, Wetzstein 2018): the Wiener-filtered
inversion of the confocal measurement operator, on the lattice f-k migration uses.  With v = r^2 (r the half path) a
confocal row obeys

    r^3 tau(x', z', r) = integral rho(x, z, sqrt(u)) / (2 sqrt(u)) delta(rho_lat^2 + u - v) dx dz du,

a 3-D convolution with a paraboloid in (x, z, v), so a Wiener deconvolution with a noise knob (snr) inverts it where
f-k migration has no knob and filtered back-projection only sharpens.  This is the project's own discretisation, not
a port of the published code (include/nlosgr.h states every formula):

    rows [H W, nr] -> psi = max(rows, 0) r^power -> g = R psi on nv depth-squared cells,
                      zero-padded to [2H, 2W, 2nv]                                              nlosgr_lct_load
                   -> S = fftn(pad)                                                             torch.fft
    K = the light cone, two non-zeros per (z, x) offset, unit norm                              nlosgr_lct_kernel
                   -> Fk = fftn(K)                                                              torch.fft
                   -> G = conj(Fk) / (|Fk|^2 + 1 / snr)   (conj(Fk) with backprop),  S G        nlosgr_lct_filter
                   -> o = ifftn(S G)                                                            torch.fft
                   -> volume[n, j, m] = max((R^T Re o)[m, n, j], 0), [W, nr, H]                 nlosgr_lct_store

R [nv, nr] resamples between time bins and cells of equal width in r^2 (lct_resampling): the share of a cell inside
a bin over the cell's mean radius, built in float64 and passed to the kernels as run tables.  The convolution is
shift-invariant in v, so a window that starts at any bin needs no special handling.  G depends on the lattice and
the window alone: lct_inverse builds it once and lct_reconstruct(..., inverse=G) reuses it for the next capture.

Lattice point (m, n) is measured at (xs[n], y0, zs[m]); voxel (n, j, m) of the result is the point (xs[n],
y0 + r0 + j dr, zs[m]) (fk.fk_grid), as for f-k migration.  The FFTs are plumbing (torch's hipFFT); everything
between them is HIP (csrc/nlosgr_lct.hip).  Bitwise repeatable; the rows may be in any order (perm=).  Confocal only:
a non-confocal capture goes to nlosgr.phasor or nlosgr.backproject.

No CPU fallback, no backward.

    python -m nlosgr.lct CAPTURE.mat --start S --end E [--power P] [--snr X] [--nv N] [--backprop] --out lct.npz
        [--mesh lct.ply --level-frac F]
"""
import argparse
import functools

import numpy as np
import torch

from . import _lib
from .fk import X_ALONG, _extents, _gpu, _inside, _work, fk_grid, lattice_spacing, wall_lattice
from .voxelize import front_view

MAX_CELLS = 2048
MODE_WIENER, MODE_BACKPROP, MODE_GIVEN = 0, 1, 2


def _f32(v):
    return float(np.float32(v))


def _cells(nv, nr):
    nv = int(nr) if nv is None else int(nv)
    if not 1 <= nv <= MAX_CELLS:
        raise ValueError(f"nlosgr: the LCT cell count nv must be in 1..{MAX_CELLS}")
    return nv


class Resampling:
    """The operator R [nv, nr] of lct_resampling as run tables (CPU tensors): row i of R is weight[start[i] :
    start[i + 1]] at the bins first[i], first[i] + 1, ...; first_t, start_t, weight_t are the same entries by
    column (R^T: per bin its run of cells).  first int32 [nv], start int32 [nv + 1], weight fp32 [nnz]; dv: the
    cell width in r^2 (float64)."""

    def __init__(self, r0, dr, nr, nv, dv, rows, cols):
        self.r0, self.dr, self.nr, self.nv, self.dv = r0, dr, nr, nv, dv
        self.first, self.start, self.weight = rows
        self.first_t, self.start_t, self.weight_t = cols
        self._on = {}

    @property
    def nnz(self):
        return int(self.weight.numel())

    def on(self, device):
        """The six tables on `device` (copied once)."""
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = tuple(t.to(device) for t in (self.first, self.start, self.weight, self.first_t,
                                                            self.start_t, self.weight_t))
        return self._on[device]

    def dense(self):
        """R as a dense float64 [nv, nr] tensor of the fp32 weights (checks, and the torch composition of the
        benchmark)."""
        R = torch.zeros((self.nv, self.nr), dtype=torch.float64)
        for i in range(self.nv):
            n = int(self.start[i + 1] - self.start[i])
            R[i, int(self.first[i]):int(self.first[i]) + n] = self.weight[int(self.start[i]):int(self.start[i + 1])].double()
        return R


def _runs(R, mask):
    """(first, start, weight) of the rows of R where mask; every row's non-zeros must be one run."""
    count = mask.sum(axis=1)
    first = np.where(count > 0, mask.argmax(axis=1), 0)
    last = mask.shape[1] - 1 - mask[:, ::-1].argmax(axis=1)
    if not np.array_equal(np.where(count > 0, last - first + 1, 0), count):
        raise RuntimeError("nlosgr: a row of the LCT resampling operator is not one contiguous run")
    start = np.concatenate([[0], np.cumsum(count)])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt))
    return t(first, np.int32), t(start, np.int32), t(R[mask], np.float32)


def lct_resampling(r0, dr, nr, nv=None):
    """The resampling between the nr time bins of a window (r0: radius of bin 0, dr: bin width, taken as the fp32
    values the kernels get) and nv cells of equal width in v = r^2 (default nr; 1..2048), a `Resampling`.  Bin j owns
    r in [e_j, e_j+1), e_j = r0 + (j - 1/2) dr with e_0 clamped at 0; dv = (e_nr^2 - e_0^2) / nv; cell i owns
    r in [t_i, t_i+1), t_i = sqrt(e_0^2 + i dv);  R[i, j] = |cell i n bin j| / (t_i+1 - t_i) / ((t_i + t_i+1) / 2).
    Built in float64, the weights rounded to fp32.  The last few results are kept: the captures of one setup share
    their window, and the dense float64 build costs more than the kernels that use it."""
    _, _, nr = _extents(1, 1, nr)
    nv = _cells(nv, nr)
    r0, dr = _f32(r0), _f32(dr)
    if not (dr > 0 and np.isfinite(dr)):
        raise ValueError("nlosgr: dr must be > 0")
    if not (r0 >= 0 and np.isfinite(r0)):
        raise ValueError("nlosgr: r0 must be >= 0")
    return _build_resampling(r0, dr, nr, nv)


@functools.lru_cache(maxsize=8)
def _build_resampling(r0, dr, nr, nv):
    e = r0 + (np.arange(nr + 1, dtype=np.float64) - 0.5) * dr
    e[0] = max(e[0], 0.0)
    v_lo, v_hi = e[0] ** 2, e[nr] ** 2
    dv = (v_hi - v_lo) / nv
    if not (dv > 0 and np.isfinite(dv)):
        raise ValueError("nlosgr: the window is too narrow to split into depth-squared cells")
    t = np.sqrt(v_lo + np.arange(nv + 1, dtype=np.float64) * dv)
    t[0], t[nv] = e[0], e[nr]
    overlap = np.minimum(t[1:, None], e[None, 1:]) - np.maximum(t[:-1, None], e[None, :-1])
    mask = overlap > 0
    R = np.where(mask, overlap, 0.0) / (t[1:] - t[:-1])[:, None] / ((t[:-1] + t[1:]) / 2)[:, None]
    return Resampling(r0, dr, nr, nv, float(dv), _runs(R, mask), _runs(np.ascontiguousarray(R.T), mask.T))


def _resampling(res, r0, dr, nr, nv):
    if res is None:
        return lct_resampling(r0, dr, nr, nv)
    if not isinstance(res, Resampling) or res.nr != int(nr) or (nv is not None and res.nv != int(nv)):
        raise ValueError("nlosgr: resampling must be lct_resampling's result for this nr and nv")
    return res


@torch.no_grad()
def lct_load(rows, H, W, r0, dr, power=4, nv=None, perm=None, x_along="n", resampling=None, out=None):
    """Stage 1, complex64 [2H, 2W, 2nv]: the rows weighted by r^power, resampled to the depth-squared cells and
    zero-padded (nlosgr_lct_load; every element of `out` is written).  perm: int32 [H W], the row that holds lattice
    point v (None: row v).  resampling: lct_resampling(r0, dr, nr, nv), built when not given."""
    lib = _lib.load()
    rows = _gpu(rows, torch.float32, "lct_load")
    if rows.dim() != 2:
        raise ValueError("nlosgr: lct_load takes rows [H W, nr]")
    H, W, nr = _extents(H, W, rows.shape[1])
    if rows.shape[0] != H * W:
        raise ValueError(f"nlosgr: rows must be [{H * W}, nr] for an {H} x {W} lattice")
    if x_along not in X_ALONG:
        raise ValueError(f"nlosgr: x_along must be one of {X_ALONG}")
    res = _resampling(resampling, r0, dr, nr, nv)
    dev = rows.device
    if perm is not None:
        perm = _gpu(perm, torch.int32, "lct_load (perm)")
        if perm.shape != (H * W,) or perm.device != dev:
            raise ValueError(f"nlosgr: perm must be int32 [{H * W}] on {dev}")
        if int(perm.min()) < 0 or int(perm.max()) >= H * W:
            raise ValueError("nlosgr: perm holds a row index outside [0, H W)")
    sm, sn = (W, 1) if x_along == "n" else (1, H)
    pad = _work(out, (2 * H, 2 * W, 2 * res.nv), dev, "lct_load")
    first, start, weight = res.on(dev)[:3]
    _lib.check(lib.nlosgr_lct_load(_lib.ptr(rows), _lib.ptr(perm), H, W, nr, res.nv, sm, sn, float(r0), float(dr),
                                   int(power), _lib.ptr(first), _lib.ptr(start), _lib.ptr(weight), res.nnz,
                                   _lib.ptr(pad), _lib.stream_handle(dev)))
    return pad


def lct_scale(H, W, nv, sx, sz, dv):
    """1 / ||K||_2 of the unscaled light-cone kernel, in float64 from the kernel's own formula over its 2H x 2W
    columns (the fp32 sx and sz the kernel gets)."""
    signed = lambda N: np.where(np.arange(N) < N // 2, np.arange(N), np.arange(N) - N).astype(np.float64)
    lb, lc = _f32(sx) * signed(2 * W), _f32(sz) * signed(2 * H)
    s = (lb[None, :] * lb[None, :] + lc[:, None] * lc[:, None]) / float(dv)
    k = np.floor(s)
    f = s - k
    norm2 = float(np.where(k <= nv - 1, (1.0 - f) ** 2, 0.0).sum() + np.where(k + 1 <= nv - 1, f ** 2, 0.0).sum())
    return 1.0 / np.sqrt(norm2)


def _kernel_args(H, W, nv, sx, sz, dv):
    H, W, _ = _extents(H, W, 1)
    nv = _cells(nv, None)
    if not (float(sx) > 0 and float(sz) > 0):
        raise ValueError("nlosgr: sx and sz must be > 0")
    if not (float(dv) > 0 and np.isfinite(float(dv))):
        raise ValueError("nlosgr: dv must be > 0")
    return H, W, nv


@torch.no_grad()
def lct_kernel(H, W, nv, sx, sz, dv, out=None, device="cuda"):
    """Stage 2, complex64 [2H, 2W, 2nv]: the light cone K with unit norm (nlosgr_lct_kernel; every element of `out`
    is written).  dv: lct_resampling(...).dv."""
    lib = _lib.load()
    H, W, nv = _kernel_args(H, W, nv, sx, sz, dv)
    dev = out.device if isinstance(out, torch.Tensor) else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("nlosgr: lct_kernel needs a GPU (no CPU fallback)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    K = _work(out, (2 * H, 2 * W, 2 * nv), dev, "lct_kernel")
    _lib.check(lib.nlosgr_lct_kernel(H, W, nv, float(sx), float(sz), float(dv), lct_scale(H, W, nv, sx, sz, dv),
                                     _lib.ptr(K), _lib.stream_handle(dev)))
    return K


def _spectrum(t, what):
    t = _gpu(t, torch.complex64, what)
    if t.dim() != 3 or any(int(n) % 2 for n in t.shape):
        raise ValueError(f"nlosgr: {what} takes a spectrum [2H, 2W, 2nv]")
    H, W, _ = _extents(int(t.shape[0]) // 2, int(t.shape[1]) // 2, 1)
    return t, H, W, _cells(int(t.shape[2]) // 2, None)


def _filter(kf, spec, snr, mode, out, what):
    lib = _lib.load()
    kf, H, W, nv = _spectrum(kf, what)
    if mode == MODE_WIENER and not (float(snr) > 0 and np.isfinite(float(snr))):
        raise ValueError("nlosgr: snr must be > 0")
    if spec is not None:
        spec = _gpu(spec, torch.complex64, what)
        if spec.shape != kf.shape or spec.device != kf.device:
            raise ValueError(f"nlosgr: the spectrum and the kernel's must both be {tuple(kf.shape)} on {kf.device}")
    out = _work(out, kf.shape, kf.device, what)
    _lib.check(lib.nlosgr_lct_filter(_lib.ptr(kf), _lib.ptr(spec), H, W, nv, float(snr), mode, _lib.ptr(out),
                                     _lib.stream_handle(kf.device)))
    return out


@torch.no_grad()
def lct_filter(spec, kf=None, inverse=None, snr=0.8, backprop=False, out=None):
    """Stage 4, complex64 [2H, 2W, 2nv]: spec G (nlosgr_lct_filter), with G formed from the kernel's spectrum
    kf = fftn(lct_kernel(...)) as conj(kf) / (|kf|^2 + 1 / snr) (conj(kf) with backprop), or given as inverse=
    (lct_inverse); exactly one of the two.  Both routes give the same bits.  out may be spec (in place).  spec None
    (with kf=): G itself."""
    if (kf is None) == (inverse is None):
        raise ValueError("nlosgr: lct_filter takes the kernel's spectrum kf= or an inverse=, one of them")
    if inverse is not None:
        if spec is None:
            raise ValueError("nlosgr: lct_filter applies an inverse= to a spectrum: spec is None")
        return _filter(inverse, spec, 1.0, MODE_GIVEN, out, "lct_filter")
    return _filter(kf, spec, snr, MODE_BACKPROP if backprop else MODE_WIENER, out, "lct_filter")


@torch.no_grad()
def lct_inverse(H, W, nv, sx, sz, dv, snr, backprop=False, device="cuda"):
    """G, complex64 [2H, 2W, 2nv]: the Wiener inverse conj(Fk) / (|Fk|^2 + 1 / snr) of the light cone's spectrum
    Fk = fftn(lct_kernel(...)), or conj(Fk) with backprop.  It depends on the lattice and the window alone: pass
    it to lct_reconstruct(inverse=) for every capture that shares them."""
    if not backprop and not (float(snr) > 0 and np.isfinite(float(snr))):
        raise ValueError("nlosgr: snr must be > 0")
    kf = torch.fft.fftn(lct_kernel(H, W, nv, sx, sz, dv, device=device))
    return lct_filter(None, kf=kf, snr=snr, backprop=backprop, out=kf)


@torch.no_grad()
def lct_store(field, resampling):
    """Stage 6, fp32 [W, nr, H]: max(R^T Re field, 0) of the [0:H, 0:W, 0:nv] corner of field [2H, 2W, 2nv] =
    ifftn(spec G), with the (cell -> bin, time <-> z) transpose into the voxel order (nlosgr_lct_store)."""
    lib = _lib.load()
    field, H, W, nv = _spectrum(field, "lct_store")
    if not isinstance(resampling, Resampling) or resampling.nv != nv:
        raise ValueError(f"nlosgr: resampling must be lct_resampling's result with nv = {nv}")
    nr = resampling.nr
    first_t, start_t, weight_t = resampling.on(field.device)[3:]
    vol = torch.empty((W, nr, H), dtype=torch.float32, device=field.device)
    _lib.check(lib.nlosgr_lct_store(_lib.ptr(field), H, W, nr, nv, _lib.ptr(first_t), _lib.ptr(start_t),
                                    _lib.ptr(weight_t), resampling.nnz, _lib.ptr(vol), _lib.stream_handle(field.device)))
    return vol


@torch.no_grad()
def lct_reconstruct(rows, H, W, sx, sz, r0, dr, power=4, snr=0.8, nv=None, backprop=False, perm=None, x_along="n",
                    inverse=None):
    """[W, nr, H] fp32: the light-cone transform of rows [H W, nr], the lattice, perm, x_along, r0, dr and power as
    for fk.fk_migrate.  snr > 0: the Wiener filter's signal-to-noise ratio (small: smooth, large: sharp and noisy);
    nv: depth-squared cells, default nr (more resolve the near bins, which are wide in r^2); backprop: apply the
    adjoint conj(Fk) instead of the Wiener inverse.  inverse: lct_inverse's result for this lattice and window
    (snr and backprop are then its own)."""
    if not (float(sx) > 0 and float(sz) > 0):
        raise ValueError("nlosgr: sx and sz must be > 0")
    if inverse is None and not backprop and not (float(snr) > 0 and np.isfinite(float(snr))):
        raise ValueError("nlosgr: snr must be > 0")
    rows = _gpu(rows, torch.float32, "lct_reconstruct")
    if rows.dim() != 2:
        raise ValueError("nlosgr: lct_reconstruct takes rows [H W, nr]")
    res = lct_resampling(r0, dr, rows.shape[1], nv)
    work = lct_load(rows, H, W, r0, dr, power=power, perm=perm, x_along=x_along, resampling=res)
    if inverse is None:
        inverse = lct_inverse(H, W, res.nv, sx, sz, res.dv, snr, backprop=backprop, device=rows.device)
    elif not isinstance(inverse, torch.Tensor) or tuple(inverse.shape) != tuple(work.shape):
        raise ValueError(f"nlosgr: inverse must be lct_inverse's complex64 {tuple(work.shape)} tensor")
    spec = torch.fft.fftn(work)
    del work
    spec = lct_filter(spec, inverse=inverse, out=spec)
    return lct_store(torch.fft.ifftn(spec), res)


@torch.no_grad()
def lct_capture(data_kwargs, start, end, power=4, snr=0.8, nv=None, backprop=False, crop=True, inverse=None):
    """The light-cone transform of the capture in data_kwargs (data.make_data_kwargs, shuffled or not) over bins
    [floor(start), floor(start) + end - start).  crop: keep the voxels inside the capture's volume box, as
    fk.fk_capture does.  Returns {"volume" [nx,ny,nz], "front", "depth" (voxelize.front_view), "grid"}, the keys of
    fk_capture.  A non-confocal capture raises NotImplementedError; a wall that is no lattice, wall_lattice's
    ValueError."""
    from .data import is_confocal, volume_target
    if not is_confocal(data_kwargs):
        raise NotImplementedError("nlosgr: the light-cone transform is confocal only: this capture's laser spots "
                                  "(laser_grid_positions) differ from its sensed points.  Use nlosgr.phasor (or "
                                  "nlosgr.backproject), which take the laser spots")
    I1 = int(np.floor(start))
    nr = int(end - start)
    H, W, xs, zs, y0, perm, x_along = wall_lattice(data_kwargs)
    _extents(H, W, nr)
    rows = volume_target(data_kwargs, start, nr)
    cdt = float(data_kwargs["c"]) * float(data_kwargs["deltaT"])
    sx = lattice_spacing(xs, None if len(xs) > 1 else lattice_spacing(zs))
    sz = lattice_spacing(zs, sx)
    vol = lct_reconstruct(rows, H, W, sx, sz, I1 * cdt, cdt, power=power, snr=snr, nv=nv, backprop=backprop,
                          perm=perm.to(rows.device), x_along=x_along, inverse=inverse)
    grid = fk_grid(xs, zs, y0, I1 * cdt, cdt, nr)
    if crop:
        vp = [float(v) for v in data_kwargs["volume_position"]]
        h = float(data_kwargs["volume_size"]) / 2
        rx, ry, rz = (_inside(t.numpy(), p - h, p + h) for t, p in zip(grid.tables, vp))
        vol = vol[rx[0]:rx[1], ry[0]:ry[1], rz[0]:rz[1]].contiguous()
        grid = grid.slice(rx, ry, rz)
    front, depth = front_view(vol, grid)
    return {"volume": vol, "front": front, "depth": depth, "grid": grid}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nlosgr.lct",
                                 description="Light-cone transform of a confocal capture on its own wall x time "
                                             "lattice (volume, front view, depth).")
    ap.add_argument("capture", help="Zaragoza-format .mat file")
    ap.add_argument("--start", type=int, required=True, help="first time bin")
    ap.add_argument("--end", type=int, required=True, help="one past the last time bin")
    ap.add_argument("--power", type=int, default=4, choices=range(5), help="falloff compensation r^power")
    ap.add_argument("--snr", type=float, default=0.8, help="signal-to-noise ratio of the Wiener filter")
    ap.add_argument("--nv", type=int, default=None, help="depth-squared cells (default: the number of bins)")
    ap.add_argument("--backprop", action="store_true", help="apply the adjoint, not the Wiener inverse")
    ap.add_argument("--out", default="lct.npz")
    ap.add_argument("--mesh", default=None, help="also write the isosurface as a PLY file")
    ap.add_argument("--level-frac", type=float, default=0.5, help="isosurface level as a fraction of the maximum")
    a = ap.parse_args(argv)
    if a.end <= a.start:
        ap.error("--end must be greater than --start")
    if not a.snr > 0:
        ap.error("--snr must be greater than 0")
    if a.nv is not None and not 1 <= a.nv <= MAX_CELLS:
        ap.error(f"--nv must be in 1..{MAX_CELLS}")
    return a


def main(argv=None):
    a = parse_args(argv)
    from .data import make_data_kwargs
    if not torch.cuda.is_available():
        raise RuntimeError("nlosgr: the light-cone transform needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    dk, *_ = make_data_kwargs(a.capture, dev, shuffle=False)
    out = lct_capture(dk, a.start, a.end, power=a.power, snr=a.snr, nv=a.nv, backprop=a.backprop)
    grid, vol = out["grid"], out["volume"]
    vp = dk["volume_position"].cpu().numpy().astype(np.float32)
    # the key names of python -m nlosgr.fk
    np.savez_compressed(a.out, density=vol.cpu().numpy(), albedo=vol.cpu().numpy(), front=out["front"].cpu().numpy(),
                        depth=out["depth"].cpu().numpy(), xs=grid.xs.numpy(), ys=grid.ys.numpy(), zs=grid.zs.numpy(),
                        cam=np.array([vp[0], 0.0, vp[2]], dtype=np.float32))
    print(f"wrote {a.out}: {grid.shape} voxels, {dk['camera_grid_positions'].shape[1]} wall points, bins "
          f"[{a.start}, {a.end}), power {a.power}, {'back-projection' if a.backprop else f'snr {a.snr:g}'}")
    if a.mesh:
        from .mesh import isosurface, write_ply
        level = a.level_frac * float(vol.max())
        mesh = isosurface(vol, grid, level)
        write_ply(a.mesh, mesh)
        print(f"wrote {a.mesh}: level {level:.6g}, {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} triangles")


if __name__ == "__main__":
    main()
