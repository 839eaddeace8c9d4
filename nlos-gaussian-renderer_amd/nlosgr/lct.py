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

The same parts run the other way give the confocal measurement operator itself, A: volume [W, nr, H] -> rows, and
its exact adjoint (LctOperator; include/nlosgr.h, "LCT operator pair"):

    A v   = w . R^T Re ifftn( fftn(pad R v) Fk )                lct_load_volume, lct_filter, lct_store_rows
    A^T h =     R^T Re ifftn( fftn(pad R (w . h)) conj(Fk) )    lct_load_rows, lct_filter, lct_store_volume

with w_j = (r0 + j dr)^power, power -4..4, and nothing clamped, so both take a residual.  LctOperator.project is
differentiable (its backward is the adjoint); lct_solve runs projected Landweber or FISTA steps on 1/2 |A v - h|^2 at
FFT speed on the capture's full lattice, lct_solve_capture does so for a loaded capture, and
voxel_fit.VoxelFitStep(operator=) fits Gaussians through it.  lct_solve_pd adds what a real capture needs: total
variation, sparsity and a Poisson data term with the falloff as a per-bin exposure, by a primal-dual iteration
(nlosgr.prox: three more HIP passes around the same operator pair).  Not built: the non-confocal case.

No CPU fallback.

    python -m nlosgr.lct CAPTURE.mat --start S --end E [--power P] [--snr X] [--nv N] [--backprop] --out lct.npz
        [--mesh lct.ply --level-frac F] [--iterations N [--no-accelerate] [--falloff Q]
        [--tv T] [--l1 L] [--loss mse|poisson] [--rate-floor E] [--gt-times G]]
"""
import functools

import numpy as np
import torch

from . import _cli, _lib
from .lattice import _extents, _f32, _gpu, _work, capture_result, confocal_lattice, fk_grid, lattice_rows

MAX_CELLS = 2048
MODE_WIENER, MODE_BACKPROP, MODE_GIVEN = 0, 1, 2
# LctOperator.norm() is a power iteration: it approaches |A|^2 from below, and the primal-dual steps need a bound from
# above.  The float64 power iteration run to convergence (1e-12) on the test lattices is at most 1.000136 times its
# 8-iteration estimate (the windows that start at bin 35; 1.00002 or less on the others): rounded up to 1.01.
NORM_SAFETY = 1.01


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


def _load(symbol, what, rows, H, W, r0, dr, power, nv, perm, x_along, resampling, out):
    """lct_load and lct_load_rows: the two instances of one kernel."""
    lib = _lib.load()
    rows = _gpu(rows, torch.float32, what)
    if rows.dim() != 2:
        raise ValueError(f"nlosgr: {what} takes rows [H W, nr]")
    H, W, nr = _extents(H, W, rows.shape[1])
    if rows.shape[0] != H * W:
        raise ValueError(f"nlosgr: rows must be [{H * W}, nr] for an {H} x {W} lattice")
    res = _resampling(resampling, r0, dr, nr, nv)
    dev = rows.device
    perm, sm, sn = lattice_rows(perm, x_along, H, W, dev, what)
    pad = _work(out, (2 * H, 2 * W, 2 * res.nv), dev, what)
    first, start, weight = res.on(dev)[:3]
    _lib.check(getattr(lib, symbol)(_lib.ptr(rows), _lib.ptr(perm), H, W, nr, res.nv, sm, sn, float(r0), float(dr),
                                    int(power), _lib.ptr(first), _lib.ptr(start), _lib.ptr(weight), res.nnz,
                                    _lib.ptr(pad), _lib.stream_handle(dev)))
    return pad


@torch.no_grad()
def lct_load(rows, H, W, r0, dr, power=4, nv=None, perm=None, x_along="n", resampling=None, out=None):
    """Stage 1, complex64 [2H, 2W, 2nv]: the rows weighted by r^power, resampled to the depth-squared cells and
    zero-padded (nlosgr_lct_load; every element of `out` is written).  perm: int32 [H W], the row that holds lattice
    point v (None: row v).  resampling: lct_resampling(r0, dr, nr, nv), built when not given."""
    return _load("nlosgr_lct_load", "lct_load", rows, H, W, r0, dr, power, nv, perm, x_along, resampling, out)


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


def _store(symbol, what, field, resampling):
    """lct_store and lct_store_volume: the two instances of one kernel."""
    lib = _lib.load()
    field, H, W, nv = _spectrum(field, what)
    if not isinstance(resampling, Resampling) or resampling.nv != nv:
        raise ValueError(f"nlosgr: resampling must be lct_resampling's result with nv = {nv}")
    nr = resampling.nr
    first_t, start_t, weight_t = resampling.on(field.device)[3:]
    vol = torch.empty((W, nr, H), dtype=torch.float32, device=field.device)
    _lib.check(getattr(lib, symbol)(_lib.ptr(field), H, W, nr, nv, _lib.ptr(first_t), _lib.ptr(start_t),
                                    _lib.ptr(weight_t), resampling.nnz, _lib.ptr(vol),
                                    _lib.stream_handle(field.device)))
    return vol


@torch.no_grad()
def lct_store(field, resampling):
    """Stage 6, fp32 [W, nr, H]: max(R^T Re field, 0) of the [0:H, 0:W, 0:nv] corner of field [2H, 2W, 2nv] =
    ifftn(spec G), with the (cell -> bin, time <-> z) transpose into the voxel order (nlosgr_lct_store)."""
    return _store("nlosgr_lct_store", "lct_store", field, resampling)


# ---- the operator pair: A (volume -> rows) and its adjoint, nothing clamped ---------------------------------------

def _power(power):
    if not -4 <= int(power) <= 4:
        raise ValueError(f"nlosgr: the LCT operator's power must be in -4..4, got {int(power)}")
    return int(power)


@torch.no_grad()
def lct_load_rows(rows, H, W, r0, dr, power=0, nv=None, perm=None, x_along="n", resampling=None, out=None):
    """lct_load for signed rows, complex64 [2H, 2W, 2nv]: R (w rows), w_j = (r0 + j dr)^power with power in -4..4
    (0 where r <= 0 and power < 0), no clamp (nlosgr_lct_load_rows).  For power 0..4 and rows >= 0 the bits of
    lct_load.  The first stage of the adjoint."""
    return _load("nlosgr_lct_load_rows", "lct_load_rows", rows, H, W, r0, dr, _power(power), nv, perm, x_along,
                 resampling, out)


@torch.no_grad()
def lct_store_volume(field, resampling):
    """lct_store without the clamp, fp32 [W, nr, H]: R^T Re field, signed (nlosgr_lct_store_volume).  Where the sum
    is >= 0 the bits of lct_store.  The last stage of the adjoint."""
    return _store("nlosgr_lct_store_volume", "lct_store_volume", field, resampling)


@torch.no_grad()
def lct_load_volume(volume, resampling, out=None):
    """The first stage of A, complex64 [2H, 2W, 2nv]: the volume [W, nr, H] resampled along its bins to the
    depth-squared cells, g[m, n, i] = sum_j R[i, j] volume[n, j, m], transposed into the work array's order and
    zero-padded (nlosgr_lct_load_volume; every element of `out` is written).  Signed, no weight."""
    lib = _lib.load()
    volume = _gpu(volume, torch.float32, "lct_load_volume")
    if volume.dim() != 3:
        raise ValueError("nlosgr: lct_load_volume takes a volume [W, nr, H]")
    H, W, nr = _extents(volume.shape[2], volume.shape[0], volume.shape[1])
    if not isinstance(resampling, Resampling) or resampling.nr != nr:
        raise ValueError(f"nlosgr: resampling must be lct_resampling's result with nr = {nr}")
    dev = volume.device
    pad = _work(out, (2 * H, 2 * W, 2 * resampling.nv), dev, "lct_load_volume")
    first, start, weight = resampling.on(dev)[:3]
    _lib.check(lib.nlosgr_lct_load_volume(_lib.ptr(volume), H, W, nr, resampling.nv, _lib.ptr(first), _lib.ptr(start),
                                          _lib.ptr(weight), resampling.nnz, _lib.ptr(pad), _lib.stream_handle(dev)))
    return pad


@torch.no_grad()
def lct_store_rows(field, resampling, power=0, perm=None, x_along="n", out=None):
    """The last stage of A, fp32 [H W, nr]: rows[v(m, n), j] = w_j sum_i R[i, j] Re field[m, n, i] over the
    [0:H, 0:W, 0:nv] corner of field [2H, 2W, 2nv], w_j = (r0 + j dr)^power with the resampling's own r0 and dr, power
    in -4..4 (nlosgr_lct_store_rows).  Signed.  perm, x_along: as lct_load; a row of `out` that no lattice point
    names is left as it is."""
    lib = _lib.load()
    field, H, W, nv = _spectrum(field, "lct_store_rows")
    if not isinstance(resampling, Resampling) or resampling.nv != nv:
        raise ValueError(f"nlosgr: resampling must be lct_resampling's result with nv = {nv}")
    nr, dev = resampling.nr, field.device
    perm, sm, sn = lattice_rows(perm, x_along, H, W, dev, "lct_store_rows")
    if out is None:
        rows = torch.empty((H * W, nr), dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_contiguous():
            raise ValueError(f"nlosgr: out must be a contiguous float32 [{H * W}, {nr}] tensor on {dev}")
        rows = _gpu(out, torch.float32, "lct_store_rows")
        if tuple(rows.shape) != (H * W, nr) or rows.device != dev:
            raise ValueError(f"nlosgr: out must be a contiguous float32 [{H * W}, {nr}] tensor on {dev}")
    first_t, start_t, weight_t = resampling.on(dev)[3:]
    _lib.check(lib.nlosgr_lct_store_rows(_lib.ptr(field), _lib.ptr(perm), H, W, nr, nv, sm, sn, resampling.r0,
                                         resampling.dr, _power(power), _lib.ptr(first_t), _lib.ptr(start_t),
                                         _lib.ptr(weight_t), resampling.nnz, _lib.ptr(rows), _lib.stream_handle(dev)))
    return rows


class LctOperator:
    """The confocal measurement operator on a wall lattice, A: volume [W, nr, H] -> rows [H W, nr], and its exact
    adjoint, at FFT speed (include/nlosgr.h, "LCT operator pair"):

        A v   = w . R^T Re ifftn( fftn(pad R v) Fk )            lct_load_volume, lct_filter, lct_store_rows
        A^T h =     R^T Re ifftn( fftn(pad R (w . h)) conj(Fk) )  lct_load_rows, lct_filter, lct_store_volume

    with w_j = (r0 + j dr)^power, power in -4..4, and nothing clamped, so both take a residual.  The lattice, the
    window, perm and x_along are lct_reconstruct's.  The resampling and the light cone's spectrum Fk (complex64
    [2H, 2W, 2nv]: 1 GiB at 128 x 128 x 1024) are built once, and one work array of that size is kept; each call
    holds one more for the spectrum while it runs.  With power = -3, scale_to_physical * A is forward_project's
    confocal transient at power -4 on grid() (the cells are not hat splats: smooth volumes agree, a single voxel
    does not)."""

    def __init__(self, H, W, sx, sz, r0, dr, nr, power=0, nv=None, perm=None, x_along="n", device="cuda"):
        self.H, self.W, self.nr = _extents(H, W, nr)
        if not (float(sx) > 0 and float(sz) > 0):
            raise ValueError("nlosgr: sx and sz must be > 0")
        self.power = _power(power)
        self.resampling = lct_resampling(r0, dr, nr, nv)
        self.nv, self.r0, self.dr = self.resampling.nv, float(r0), float(dr)   # (the kernels take them as fp32)
        self.sx, self.sz = float(sx), float(sz)
        self.work = lct_kernel(self.H, self.W, self.nv, sx, sz, self.resampling.dv, device=device)
        self.device = self.work.device
        self.Fk = torch.fft.fftn(self.work)
        self.perm, _, _ = lattice_rows(perm, x_along, self.H, self.W, self.device, "LctOperator")
        self.x_along = x_along

    @property
    def volume_shape(self):
        return (self.W, self.nr, self.H)

    @property
    def rows_shape(self):
        return (self.H * self.W, self.nr)

    @property
    def scale_to_physical(self):
        """dv / (2 dr lct_scale): scale_to_physical * A at power -3 is forward_project at power -4, per unit voxel
        value (the resampling carries one 1 / r, the cell width dv / (2 r) the bin's share, lct_scale the kernel's
        unit norm)."""
        dv = self.resampling.dv
        return dv / (2.0 * self.resampling.dr * lct_scale(self.H, self.W, self.nv, self.sx, self.sz, dv))

    def grid(self, xs, zs, y0):
        """The VoxelGrid of the operator's volumes (fk.fk_grid, from r0 and dr as they were given)."""
        return fk_grid(xs, zs, y0, self.r0, self.dr, self.nr)

    @torch.no_grad()
    def forward(self, volume, out=None):
        """A volume: rows [H W, nr] fp32, signed."""
        volume = _gpu(volume, torch.float32, "LctOperator.forward")
        if tuple(volume.shape) != self.volume_shape or volume.device != self.device:
            raise ValueError(f"nlosgr: the volume must be float32 {self.volume_shape} on {self.device}")
        spec = torch.fft.fftn(lct_load_volume(volume, self.resampling, out=self.work))
        lct_filter(spec, inverse=self.Fk, out=spec)
        return lct_store_rows(torch.fft.ifftn(spec, out=self.work), self.resampling, power=self.power, perm=self.perm,
                              x_along=self.x_along, out=out)

    @torch.no_grad()
    def adjoint(self, rows):
        """A^T rows: a volume [W, nr, H] fp32, signed."""
        rows = _gpu(rows, torch.float32, "LctOperator.adjoint")
        if tuple(rows.shape) != self.rows_shape or rows.device != self.device:
            raise ValueError(f"nlosgr: the rows must be float32 {self.rows_shape} on {self.device}")
        spec = torch.fft.fftn(lct_load_rows(rows, self.H, self.W, self.r0, self.dr, power=self.power, perm=self.perm,
                                            x_along=self.x_along, resampling=self.resampling, out=self.work))
        lct_filter(spec, kf=self.Fk, backprop=True, out=spec)
        return lct_store_volume(torch.fft.ifftn(spec, out=self.work), self.resampling)

    def project(self, volume):
        """forward as a differentiable function of the volume; the backward is adjoint of the upstream rows."""
        return _LctProjectFn.apply(volume, self)

    @torch.no_grad()
    def norm(self, iterations=8):
        """The largest eigenvalue of A^T A by power iteration from the all-ones volume, as
        forward_project.operator_norm: a float, one host read at the end.  1 / norm is lct_solve's step."""
        if int(iterations) < 1:
            raise ValueError("nlosgr: iterations must be >= 1")
        v = torch.ones(self.volume_shape, device=self.device)
        lam = None
        for _ in range(int(iterations)):
            v = v / v.double().norm().float()
            v = self.adjoint(self.forward(v))
            lam = v.double().norm()
        return float(lam)


class _LctProjectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, volume, op):
        ctx.op = op
        return op.forward(volume)

    @staticmethod
    def backward(ctx, grad_rows):
        return ctx.op.adjoint(grad_rows), None


def lct_project(volume, H, W, sx, sz, r0, dr, power=0, nv=None, perm=None, x_along="n"):
    """A volume in one call: LctOperator(H, W, sx, sz, r0, dr, nr, ...).forward(volume) for a volume [W, nr, H]."""
    volume = _gpu(volume, torch.float32, "lct_project")
    if volume.dim() != 3:
        raise ValueError("nlosgr: lct_project takes a volume [W, nr, H]")
    return LctOperator(H, W, sx, sz, r0, dr, volume.shape[1], power=power, nv=nv, perm=perm, x_along=x_along,
                       device=volume.device).forward(volume)


def lct_adjoint(rows, H, W, sx, sz, r0, dr, power=0, nv=None, perm=None, x_along="n"):
    """A^T rows in one call: LctOperator(...).adjoint(rows) for rows [H W, nr]."""
    rows = _gpu(rows, torch.float32, "lct_adjoint")
    if rows.dim() != 2:
        raise ValueError("nlosgr: lct_adjoint takes rows [H W, nr]")
    return LctOperator(H, W, sx, sz, r0, dr, rows.shape[1], power=power, nv=nv, perm=perm, x_along=x_along,
                       device=rows.device).adjoint(rows)


@torch.no_grad()
def lct_solve(rows, op, iterations=30, nonneg=True, step=None, x0=None, accelerate=False):
    """(volume [W, nr, H], objective [iterations]): projected gradient on 1/2 |A v - h|^2 with A = op (an
    LctOperator), laid out like forward_project.landweber:  x+ = max(y - step A^T (A y - h), 0) (no max without
    nonneg) from x0 (zeros by default), step = 1 / op.norm() by default.  accelerate=False: y = x+ (Landweber).
    accelerate=True: FISTA, t+ = (1 + sqrt(1 + 4 t^2)) / 2, y = x+ + ((t - 1) / t+) (x+ - x), t = 1 at the start;
    the projection is applied to x+, and x+ is what is returned.
    objective[n] is 1/2 |A y_n - h|^2 at the point y_n where gradient n is taken, BEFORE update n (with FISTA that
    is the extrapolated point, not the iterate x_n); float64 on the device, no host read inside the loop."""
    if not isinstance(op, LctOperator):
        raise TypeError("nlosgr: lct_solve takes an LctOperator")
    rows = _gpu(rows, torch.float32, "lct_solve")
    if tuple(rows.shape) != op.rows_shape or rows.device != op.device:
        raise ValueError(f"nlosgr: the rows must be float32 {op.rows_shape} on {op.device}")
    step = 1.0 / op.norm() if step is None else float(step)
    if x0 is None:
        x = torch.zeros(op.volume_shape, device=rows.device)
    else:
        x = _gpu(x0, torch.float32, "lct_solve").clone()
        if tuple(x.shape) != op.volume_shape:
            raise ValueError(f"nlosgr: x0 must have the operator's volume shape {op.volume_shape}")
    objective = torch.zeros(int(iterations), dtype=torch.float64, device=rows.device)
    res = torch.empty_like(rows)
    y, t = x.clone(), 1.0
    for n in range(int(iterations)):
        op.forward(y, out=res)
        res.sub_(rows)
        objective[n] = 0.5 * res.double().square().sum()
        y.sub_(op.adjoint(res), alpha=step)                 # y is now x+
        if nonneg:
            y.clamp_(min=0.0)
        if accelerate:
            t_next = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
            x, y = y, torch.add(y, y - x, alpha=(t - 1.0) / t_next)
            t = t_next
        else:
            x = y
    return x, objective


@torch.no_grad()
def lct_solve_pd(rows, op, iterations=100, tv=0.0, l1=0.0, loss="mse", exposure=None, gt_times=1.0, rate_floor=1.0,
                 weights=(1.0, 1.0, 1.0), nonneg=True, norm=None, tau=None, sigma=None, x0=None):
    """(volume [W, nr, H], objective [iterations], terms [iterations, 3]): prox.primal_dual with A = op (an
    LctOperator), for  F(A v) + tv sum |a o grad v|_2 + l1 sum |v|  over v >= 0 (any v without nonneg).  loss "mse":
    F = 1/2 |A v - rows|^2.  loss "poisson": the rows are photon counts, F = sum [rho - y' + y' log(y'/rho)] with
    y' = max(gt_times rows, 0) + rate_floor and rho = exposure_j (A v) + rate_floor; exposure fp32 [nr] >= 0 (None:
    ones) is where a capture's falloff belongs.  tv, l1 are absolute here (lct_solve_capture scales them); weights:
    the gradient's axis weights (n, j, m).
    norm: an upper bound of |A|^2; by default NORM_SAFETY op.norm(): the power iteration bounds |A|^2 from below, and
    in float64, run to convergence on the test lattices, it ends at most 1.000136 times its 8-iteration estimate,
    which NORM_SAFETY = 1.01 rounds up.  tau, sigma: the steps, 1 / sqrt(norm + 4 sum a^2) by default (the second part
    with tv > 0 only).  objective and terms as prox.primal_dual's: float64 on the device, at the point the operator is
    applied to, before the update; no host read inside the loop."""
    from . import prox
    if not isinstance(op, LctOperator):
        raise TypeError("nlosgr: lct_solve_pd takes an LctOperator")
    rows = _gpu(rows, torch.float32, "lct_solve_pd")
    if tuple(rows.shape) != op.rows_shape or rows.device != op.device:
        raise ValueError(f"nlosgr: the rows must be float32 {op.rows_shape} on {op.device}")
    norm = NORM_SAFETY * op.norm() if norm is None else float(norm)
    z = torch.empty_like(rows)
    return prox.primal_dual(rows, lambda v: op.forward(v, out=z), op.adjoint, op.volume_shape, norm, iterations, tv=tv,
                            l1=l1, loss=loss, exposure=exposure, gt_times=gt_times, rate_floor=rate_floor,
                            weights=weights, nonneg=nonneg, tau=tau, sigma=sigma, x0=x0)


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
    c = confocal_lattice(data_kwargs, start, end, "the light-cone transform")
    vol = lct_reconstruct(c.rows, c.H, c.W, c.sx, c.sz, c.r0, c.dr, power=power, snr=snr, nv=nv, backprop=backprop,
                          perm=c.perm, x_along=c.x_along, inverse=inverse)
    return capture_result(data_kwargs, fk_grid(c.xs, c.zs, c.y0, c.r0, c.dr, c.nr), vol, crop)


@torch.no_grad()
def lct_solve_capture(data_kwargs, start, end, falloff=3, power=0, iterations=30, accelerate=True, nv=None,
                      crop=True, tv=0.0, l1=0.0, loss="mse", rate_floor=1.0, gt_times=1.0, weights=(1.0, 1.0, 1.0)):
    """The non-negative least-squares volume of a confocal capture on its own lattice: lct_solve with
    LctOperator(power=power) on the rows of bins [floor(start), floor(start) + end - start), bin j multiplied by
    (r0 + j dr)^falloff first, as voxel_fit.fit_capture does.  Returns the keys of lct_capture plus "objective"
    [iterations]; crop, and the errors (a non-confocal capture, a wall that is no lattice), as there.

    Why falloff=3 with power=0 is the default, not power=-3 on the raw rows: both state the same physical model
    (A at power -3 is the confocal transient), but at power -3 the operator carries r^-3 itself, and in a window
    that starts at r0 = 0 its first bins give it a norm of about 1e11: the step 1 / norm is then so small that the
    far voxels do not move and the solve stalls.  Moving the r^3 to the rows leaves an operator of norm about 1.

    With tv > 0, l1 > 0 or loss="poisson" the volume is lct_solve_pd's instead (accelerate is then unused), and the
    result also holds "terms" [iterations, 3] and "lambda0" (a float).  tv and l1 are fractions of
    lambda0 = max(-A^T grad F(0)), the l1 above which the zero volume is the minimiser: max A^T h for the MSE,
    max A^T (e (y'/eps - 1)) for the Poisson term; one adjoint, so the capture's scale need not be known.
    A lambda0 that comes out negative (rows with nothing above zero) is taken as 0, and tv and l1 with it.
    loss="poisson": multiplying counts by r^falloff would break their statistics, so the rows stay raw (times
    gt_times inside the likelihood) and the falloff becomes the exposure e_j = r_j^-falloff (0 where r_j <= 0,
    built in float64); eps = rate_floor.  weights: lct_solve_pd's."""
    from . import prox
    kind = prox._loss(loss)
    c = confocal_lattice(data_kwargs, start, end, "the LCT solver")
    rows = _gpu(c.rows.float(), torch.float32, "lct_solve_capture")
    radii = c.r0 + c.dr * torch.arange(c.nr, dtype=torch.float64, device=rows.device)
    exposure = None
    if kind == _lib.LOSS_POISSON:
        exposure = torch.where(radii > 0, radii.clamp(min=1e-300).pow(-float(falloff)), torch.zeros_like(radii)).float()
    elif falloff:
        rows = (rows.double() * radii.pow(float(falloff))[None]).float()
    op = LctOperator(c.H, c.W, c.sx, c.sz, c.r0, c.dr, c.nr, power=power, nv=nv, perm=c.perm, x_along=c.x_along,
                     device=rows.device)
    more = {}
    if float(tv) == 0 and float(l1) == 0 and kind == _lib.LOSS_MSE:
        vol, objective = lct_solve(rows, op, iterations=iterations, accelerate=accelerate)
    else:
        if kind == _lib.LOSS_POISSON:
            if not (float(rate_floor) > 0 and np.isfinite(float(rate_floor))):
                raise ValueError("nlosgr: rate_floor must be finite and > 0")
            pull = (rows.double().mul(float(gt_times)).clamp_(min=0.0) * (exposure.double() / float(rate_floor))[None]).float()
        else:
            pull = rows
        lambda0 = max(float(op.adjoint(pull).max()), 0.0)          # rows that pull no voxel up: no weight at all
        vol, objective, terms = lct_solve_pd(rows, op, iterations=iterations, tv=float(tv) * lambda0,
                                             l1=float(l1) * lambda0, loss=loss, exposure=exposure, gt_times=gt_times,
                                             rate_floor=rate_floor, weights=weights)
        more = {"terms": terms, "lambda0": lambda0}
    out = capture_result(data_kwargs, op.grid(c.xs, c.zs, c.y0), vol, crop)
    out["objective"] = objective
    out.update(more)
    return out


def parse_args(argv=None):
    ap = _cli.capture_parser("python -m nlosgr.lct", "lct.npz", "Light-cone transform of a confocal capture on its own "
                                                                "wall x time lattice (volume, front view, depth).")
    ap.add_argument("--power", type=int, default=None, choices=range(-4, 5),
                    help="falloff compensation r^power, 0..4 (default 4); with --iterations the operator's power, "
                         "-4..4 (default 0)")
    ap.add_argument("--snr", type=float, default=0.8, help="signal-to-noise ratio of the Wiener filter")
    ap.add_argument("--nv", type=int, default=None, help="depth-squared cells (default: the number of bins)")
    ap.add_argument("--backprop", action="store_true", help="apply the adjoint, not the Wiener inverse")
    ap.add_argument("--iterations", type=int, default=0,
                    help="N > 0: the iterative least-squares volume (lct_solve_capture, N steps on the rows times "
                         "r^falloff) instead of the Wiener filter; --power is then the operator's (0 unless given)")
    ap.add_argument("--no-accelerate", dest="accelerate", action="store_false",
                    help="with --iterations: plain Landweber steps instead of FISTA")
    ap.add_argument("--falloff", type=float, default=3.0, help="with --iterations: multiply bin j by (r0 + j dr)^falloff")
    ap.add_argument("--tv", type=float, default=0.0,
                    help="with --iterations: total-variation weight as a fraction of lambda0 (lct_solve_capture); with "
                         "--tv, --l1 or --loss poisson the primal-dual solver runs instead of FISTA")
    ap.add_argument("--l1", type=float, default=0.0, help="with --iterations: sparsity weight as a fraction of lambda0")
    ap.add_argument("--loss", choices=("mse", "poisson"), default="mse",
                    help="with --iterations: the data term; poisson takes the raw counts and --falloff as an exposure")
    ap.add_argument("--rate-floor", type=float, default=1.0, help="with --loss poisson: the rate floor eps, in counts")
    ap.add_argument("--gt-times", type=float, default=1.0, help="with --loss poisson: the factor that brings the rows to counts")
    a = _cli.parse(ap, argv)
    if a.iterations < 0:
        ap.error("--iterations must be >= 0")
    if a.power is None:
        a.power = 0 if a.iterations else 4
    if not a.iterations and a.power < 0:
        ap.error("--power must be in 0..4 without --iterations")
    if not a.snr > 0:
        ap.error("--snr must be greater than 0")
    if a.nv is not None and not 1 <= a.nv <= MAX_CELLS:
        ap.error(f"--nv must be in 1..{MAX_CELLS}")
    if not (0 <= a.tv < float("inf") and 0 <= a.l1 < float("inf")):
        ap.error("--tv and --l1 must be finite and >= 0")
    if not 0 < a.rate_floor < float("inf"):
        ap.error("--rate-floor must be finite and greater than 0")
    if not abs(a.gt_times) < float("inf"):
        ap.error("--gt-times must be finite")
    a.primal_dual = a.tv > 0 or a.l1 > 0 or a.loss != "mse"
    if a.primal_dual and not a.iterations:
        ap.error("--tv, --l1 and --loss poisson belong to --iterations")
    return a


def main(argv=None):
    a = parse_args(argv)
    dk = _cli.open_capture(a.capture, "the light-cone transform")
    if a.iterations:
        out = lct_solve_capture(dk, a.start, a.end, falloff=a.falloff, power=a.power, iterations=a.iterations,
                                accelerate=a.accelerate, nv=a.nv, tv=a.tv, l1=a.l1, loss=a.loss,
                                rate_floor=a.rate_floor, gt_times=a.gt_times)
        extra = {"objective": out["objective"].cpu().numpy()}
        how = f"{a.iterations} {'FISTA' if a.accelerate else 'Landweber'} steps, falloff {a.falloff:g}"
        if a.primal_dual:
            extra.update(terms=out["terms"].cpu().numpy(), lambda0=np.float64(out["lambda0"]))
            how = f"{a.iterations} primal-dual steps, {a.loss}, tv {a.tv:g}, l1 {a.l1:g}, falloff {a.falloff:g}"
    else:
        out = lct_capture(dk, a.start, a.end, power=a.power, snr=a.snr, nv=a.nv, backprop=a.backprop)
        extra = {}
        how = "back-projection" if a.backprop else f"snr {a.snr:g}"
    _cli.write_volume(a, dk, out, f"power {a.power}, {how}", **extra)


if __name__ == "__main__":
    main()
