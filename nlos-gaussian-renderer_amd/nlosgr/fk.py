"""f-k migration of a confocal capture (Lindell, Wetzstein, O'Toole 2019): the fast reconstruction next to
back-projection.  Where nlosgr.backproject evaluates every (voxel, wall point) pair, O(N^5) for an N^2 wall and N^3
voxels, this is a few passes over one padded array and two FFTs, O(N^3 log N); it has no SNR or wavelength knob and
serves diffuse and specular scenes alike.  The volume lives on the capture's own lattice (wall point x time bin),
not on a free voxel grid (include/nlosgr.h states every formula):

    rows [H W, nr] -> psi = sqrt(max(rows, 0) r^power) -> zero-padded to [2H, 2W, 2nr]         nlosgr_fk_load
                   -> S = fftn(pad)                                                             torch.fft
                   -> V = Stolt resampling of S along the time frequency, phase for r0          nlosgr_fk_stolt
                   -> o = ifftn(V)                                                              torch.fft
                   -> volume[n, j, m] = |o[m, n, j]|^2, [W, nr, H]                              nlosgr_fk_store

Lattice point (m, n) is measured at (xs[n], y0, zs[m]); voxel (n, j, m) of the result is the point (xs[n],
y0 + r0 + j dr, zs[m]) in the project's voxel order (fk_grid).  r0 is the radius of bin 0 and dr = c deltaT the bin
width, in half-path units as everywhere in the package.  The FFTs are plumbing (torch's hipFFT); everything between
them is HIP (csrc/nlosgr_fk.hip).  Bitwise repeatable; the rows may be in any order (perm=), so a shuffled capture
needs no gather pass.  Confocal only: a non-confocal capture goes to nlosgr.phasor or nlosgr.backproject.

No CPU fallback, no backward.

    python -m nlosgr.fk CAPTURE.mat --start S --end E [--power P] [--no-amplitude] --out fk.npz
        [--mesh fk.ply --level-frac F]
"""
import torch

from . import _cli, _lib
from .lattice import X_ALONG, fk_grid, lattice_spacing, wall_lattice   # noqa: F401  (named through this module too)
from .lattice import _extents, _gpu, _work, capture_result, confocal_lattice, lattice_rows


@torch.no_grad()
def fk_load(rows, H, W, r0, dr, power=4, amplitude=True, perm=None, x_along="n", out=None):
    """Stage 1, complex64 [2H, 2W, 2nr]: the rows as the zero-padded amplitude array (nlosgr_fk_load; every
    element of `out` is written).  perm: int32 [H W], the row that holds lattice point v (None: row v)."""
    lib = _lib.load()
    rows = _gpu(rows, torch.float32, "fk_load")
    if rows.dim() != 2:
        raise ValueError("nlosgr: fk_load takes rows [H W, nr]")
    H, W, nr = _extents(H, W, rows.shape[1])
    if rows.shape[0] != H * W:
        raise ValueError(f"nlosgr: rows must be [{H * W}, nr] for an {H} x {W} lattice")
    if not float(dr) > 0:
        raise ValueError("nlosgr: dr must be > 0")
    dev = rows.device
    perm, sm, sn = lattice_rows(perm, x_along, H, W, dev, "fk_load")
    pad = _work(out, (2 * H, 2 * W, 2 * nr), dev, "fk_load")
    _lib.check(lib.nlosgr_fk_load(_lib.ptr(rows), _lib.ptr(perm), H, W, nr, sm, sn, float(r0), float(dr), int(power),
                                  int(bool(amplitude)), _lib.ptr(pad), _lib.stream_handle(dev)))
    return pad


@torch.no_grad()
def fk_stolt(spec, sx, sz, r0, dr, out=None):
    """Stage 3, complex64 [2H, 2W, 2nr]: the Stolt-resampled spectrum of `spec` = fftn(fk_load(...))
    (nlosgr_fk_stolt; every element of `out` is written, and out may not be spec)."""
    lib = _lib.load()
    spec = _gpu(spec, torch.complex64, "fk_stolt")
    if spec.dim() != 3 or any(int(n) % 2 for n in spec.shape):
        raise ValueError("nlosgr: fk_stolt takes a spectrum [2H, 2W, 2nr]")
    H, W, nr = _extents(*(int(n) // 2 for n in spec.shape))
    out = _work(out, spec.shape, spec.device, "fk_stolt")
    if out.data_ptr() == spec.data_ptr():
        raise ValueError("nlosgr: fk_stolt cannot work in place")
    _lib.check(lib.nlosgr_fk_stolt(_lib.ptr(spec), H, W, nr, float(sx), float(sz), float(r0), float(dr), _lib.ptr(out),
                                   _lib.stream_handle(spec.device)))
    return out


@torch.no_grad()
def fk_store(field):
    """Stage 5, fp32 [W, nr, H]: |field|^2 of the [0:H, 0:W, 0:nr] corner of field [2H, 2W, 2nr] = ifftn(V), with
    the (time <-> z) transpose into the voxel order (nlosgr_fk_store)."""
    lib = _lib.load()
    field = _gpu(field, torch.complex64, "fk_store")
    if field.dim() != 3 or any(int(n) % 2 for n in field.shape):
        raise ValueError("nlosgr: fk_store takes a field [2H, 2W, 2nr]")
    H, W, nr = _extents(*(int(n) // 2 for n in field.shape))
    vol = torch.empty((W, nr, H), dtype=torch.float32, device=field.device)
    _lib.check(lib.nlosgr_fk_store(_lib.ptr(field), H, W, nr, _lib.ptr(vol), _lib.stream_handle(field.device)))
    return vol


@torch.no_grad()
def fk_migrate(rows, H, W, sx, sz, r0, dr, power=4, amplitude=True, perm=None, x_along="n"):
    """[W, nr, H] fp32: the f-k migration of rows [H W, nr], the row of lattice point v = m W + n (x_along="n") or
    v = n H + m (x_along="m") being rows[perm[v]] (perm None: rows[v]), measured at (xs[n], y0, zs[m]) with uniform
    spacings sx, sz.  r0: radius of bin 0; dr: bin width; power 0..4: the falloff compensation r^power (4: the r^-4
    of the renderer's histograms); amplitude: migrate the square root of the compensated rows."""
    if not (float(sx) > 0 and float(sz) > 0):
        raise ValueError("nlosgr: sx and sz must be > 0")
    work = fk_load(rows, H, W, r0, dr, power=power, amplitude=amplitude, perm=perm, x_along=x_along)
    spec = torch.fft.fftn(work)
    work = fk_stolt(spec, sx, sz, r0, dr, out=work)      # (the padded array has been read: its storage is reused)
    del spec
    return fk_store(torch.fft.ifftn(work))


@torch.no_grad()
def fk_capture(data_kwargs, start, end, power=4, amplitude=True, crop=True):
    """f-k migration of the capture in data_kwargs (data.make_data_kwargs, shuffled or not) over bins
    [floor(start), floor(start) + end - start).  crop: keep the voxels inside the capture's volume box
    (volume_position +- volume_size / 2), a contiguous block of the full volume with grid.slice's tables.
    Returns {"volume" [nx,ny,nz], "front", "depth" (voxelize.front_view), "grid"}, the keys of
    backproject_capture.  A non-confocal capture raises NotImplementedError."""
    c = confocal_lattice(data_kwargs, start, end, "f-k migration")
    vol = fk_migrate(c.rows, c.H, c.W, c.sx, c.sz, c.r0, c.dr, power=power, amplitude=amplitude, perm=c.perm,
                     x_along=c.x_along)
    return capture_result(data_kwargs, fk_grid(c.xs, c.zs, c.y0, c.r0, c.dr, c.nr), vol, crop)


def parse_args(argv=None):
    ap = _cli.capture_parser("python -m nlosgr.fk", "fk.npz", "f-k migration of a confocal capture on its own wall x "
                                                              "time lattice (volume, front view, depth).")
    ap.add_argument("--power", type=int, default=4, choices=range(5), help="falloff compensation r^power")
    ap.add_argument("--no-amplitude", action="store_true", help="migrate the compensated rows, not their square root")
    return _cli.parse(ap, argv)


def main(argv=None):
    a = parse_args(argv)
    dk = _cli.open_capture(a.capture, "f-k migration")
    out = fk_capture(dk, a.start, a.end, power=a.power, amplitude=not a.no_amplitude)
    _cli.write_volume(a, dk, out, f"power {a.power}, {'amplitude' if not a.no_amplitude else 'intensity'}")


if __name__ == "__main__":
    main()
