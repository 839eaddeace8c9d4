"""Phasor-field reconstruction of a confocal or non-confocal capture: a complex-valued back-projection.

The relay wall is treated as a virtual aperture lit by a virtual wave of wavelength lambda.  Every measured
row is convolved in time with a complex Morlet wavelet (the "virtual illumination": a Gaussian envelope times
exp(2 pi i t / P)), the complex rows are back-projected, and the image is the magnitude:

    y_i = h_i * (IRF_cos + i IRF_sin)                              phasor_kernel, phasor_rows
    P(x) = sum_i weight ((1-f) y_i[k] + f y_i[k+1])                phasor_backproject: nlosgr_backproject_phasor
    volume(x) = |P(x)|

The gather is one HIP pass over interleaved (re, im) rows (csrc/nlosgr_backproject.hip): the per-pair arithmetic of
backproject (lasers=None) or of its non-confocal form (lasers=) formed once and shared by both channels, one
16-byte read per (voxel, measurement) pair.  Each plane is bitwise what backproject gives for that channel alone.
On noisy or non-confocal data the image is much cleaner than filtered back-projection, because the wavelet is a
band-pass matched to what the aperture can resolve.

No CPU fallback, no backward.

    python -m nlosgr.phasor CAPTURE.mat --resolution 128 --start S --end E --wavelength L [--cycles C]
        [--power P] --out ph.npz [--mesh ph.ply --level-frac F]
"""
import ctypes
import math

import numpy as np
import torch

from . import _cli, _lib
from .backproject import _gpu_f32, _lasers_arg, capture_lasers, fp32_window
from .irf import IRF, MAX_TAPS, irf_apply
from .voxelize import VoxelGrid, front_view


def phasor_kernel(wavelength, dr, cycles=4.0):
    """(IRF_cos, IRF_sin): the real and imaginary taps of the Morlet wavelet of the virtual illumination, as two
    nlosgr.irf.IRF (apply them with phasor_rows).  wavelength: in scene length units along the WHOLE path laser
    -> x -> sensor; dr: the rows' bin width, which counts half the path as everywhere in this package, so the
    period in bins is P = wavelength / (2 dr).  The envelope is a Gaussian of sigma_b = cycles P / 6 bins (+-3
    sigma span `cycles` periods), normalised to sum 1, over taps m = -n..n with n = ceil(3 sigma_b):

        env[m] = exp(-m^2 / (2 sigma_b^2)) / sum,   cos taps env cos(2 pi m / P),   sin taps env sin(2 pi m / P)

    (float64, rounded to fp32 by IRF), centre n, background 0.  Keep the wavelength at least 2-4 spacings of the
    wall's points: below that the aperture is undersampled and the image aliases.  ValueError for P < 2 (the
    temporal Nyquist limit), cycles <= 0 or more than irf.MAX_TAPS taps."""
    wavelength, dr, cycles = float(wavelength), float(dr), float(cycles)
    if not dr > 0:
        raise ValueError("nlosgr: dr must be > 0")
    if not cycles > 0:
        raise ValueError("nlosgr: cycles must be > 0")
    P = wavelength / (2.0 * dr)
    if not P >= 2.0:
        raise ValueError(f"nlosgr: wavelength {wavelength} is {P:.3g} bins per period; the rows resolve >= 2 (Nyquist)")
    sigma = cycles * P / 6.0
    n = int(math.ceil(3.0 * sigma))
    if 2 * n + 1 > MAX_TAPS:
        raise ValueError(f"nlosgr: this wavelet needs {2 * n + 1} taps (> {MAX_TAPS}); lower cycles or the wavelength")
    m = np.arange(-n, n + 1, dtype=np.float64)
    env = np.exp(-m * m / (2.0 * sigma * sigma))
    env /= env.sum()
    ph = 2.0 * np.pi * m / P
    return IRF(env * np.cos(ph), n, 0.0), IRF(env * np.sin(ph), n, 0.0)


@torch.no_grad()
def phasor_rows(rows, kernel):
    """[nmeas, nr, 2] contiguous fp32: rows [nmeas, nr] (float32, GPU) convolved in time with both wavelets of
    `kernel` (phasor_kernel's pair), interleaved as (re, im): the layout phasor_backproject reads.  Two
    irf_apply calls (the filter is about 1 % of the gather's work)."""
    kc, ks = kernel
    return torch.stack((irf_apply(rows, kc), irf_apply(rows, ks)), dim=-1).contiguous()


@torch.no_grad()
def phasor_backproject(rows_c, walls, grid, r0, dr, power=0, lasers=None, planes=None, accumulate=False,
                       magnitude=True):
    """(planes [2, nx, ny, nz], mag [nx, ny, nz] or None): the back-projection of the complex rows rows_c
    [nmeas, nr, 2] (phasor_rows) measured at walls [nmeas, 3] onto `grid`.  planes[0] / planes[1] are bitwise
    backproject(rows_c[..., 0] / rows_c[..., 1], walls, grid, r0, dr, power, lasers=lasers); mag is
    sqrt(re^2 + im^2) formed in float64 from the fp32 planes and rounded once.  r0, dr, power, lasers: as
    backproject.  planes: a [2, nx, ny, nz] tensor to write (accumulate=False) or to add this call's sums to
    (accumulate=True: measurements in batches; mag is then the magnitude of the accumulated planes).
    magnitude=False skips mag."""
    lib = _lib.load()
    rows_c, walls = _gpu_f32(rows_c, "phasor_backproject"), _gpu_f32(walls, "phasor_backproject")
    if (rows_c.dim() != 3 or rows_c.shape[2] != 2 or walls.dim() != 2 or walls.shape[1] != 3
            or walls.shape[0] != rows_c.shape[0]):
        raise ValueError("nlosgr: phasor_backproject takes rows_c [nmeas, nr, 2] and walls [nmeas, 3]")
    if lasers is not None:
        lasers = _lasers_arg(lasers, walls, "phasor_backproject")
    if not isinstance(grid, VoxelGrid):
        raise TypeError("nlosgr: grid must be a voxelize.VoxelGrid")
    dev = rows_c.device
    shape = grid.shape
    pshape = (2,) + shape
    if planes is None:
        if accumulate:
            raise ValueError("nlosgr: accumulate=True needs the planes to add to (planes=)")
        planes = torch.empty(pshape, device=dev)
    else:
        if not isinstance(planes, torch.Tensor) or not planes.is_cuda or planes.dtype != torch.float32:
            raise RuntimeError("nlosgr: phasor_backproject needs float32 GPU tensors (no CPU fallback)")
        if tuple(planes.shape) != pshape or not planes.is_contiguous() or planes.device != dev:
            raise ValueError(f"nlosgr: planes must be a contiguous {pshape} tensor on {dev}")
    if not float(dr) > 0:
        raise ValueError("nlosgr: dr must be > 0")
    mag = torch.empty(shape, device=dev) if magnitude else None
    xs, ys, zs = grid.on(dev)
    vg = _lib.VoxelGrid(shape[0], shape[1], shape[2], _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(zs))
    opt = _lib.BackprojectOpts(*fp32_window(r0, dr), int(power), int(bool(accumulate)))
    _lib.check(lib.nlosgr_backproject_phasor(_lib.ptr(rows_c), _lib.ptr(walls), _lib.ptr(lasers),
                                             0 if lasers is None else lasers.shape[0], rows_c.shape[0],
                                             rows_c.shape[1], ctypes.byref(vg), ctypes.byref(opt), _lib.ptr(planes),
                                             _lib.ptr(mag), _lib.stream_handle(dev)))
    return planes, mag


@torch.no_grad()
def phasor_capture(data_kwargs, resolution, start, end, wavelength, cycles=4.0, power=0):
    """Phasor-field image of the capture in data_kwargs (data.make_data_kwargs) over bins [floor(start),
    floor(start) + end - start) onto VoxelGrid(volume_position, volume_size, resolution): the counterpart of
    backproject.backproject_capture.  A non-confocal capture (data_kwargs["laser_grid_positions"]) is
    reconstructed with its laser spots.  Returns {"volume" [nx,ny,nz] (the magnitude), "real", "imag", "front",
    "depth" (voxelize.front_view of the magnitude), "grid"}."""
    from .data import volume_target
    I1 = int(np.floor(start))
    rows = volume_target(data_kwargs, start, int(end - start))
    walls = data_kwargs["camera_grid_positions"].t().contiguous().float()
    cdt = float(data_kwargs["c"]) * float(data_kwargs["deltaT"])
    rows_c = phasor_rows(_gpu_f32(rows, "phasor_capture"), phasor_kernel(wavelength, cdt, cycles))
    vp = data_kwargs["volume_position"]
    grid = VoxelGrid([float(v) for v in vp], float(data_kwargs["volume_size"]), resolution)
    planes, mag = phasor_backproject(rows_c, walls, grid, I1 * cdt, cdt, power=power, lasers=capture_lasers(data_kwargs))
    front, depth = front_view(mag, grid)
    return {"volume": mag, "real": planes[0], "imag": planes[1], "front": front, "depth": depth, "grid": grid}


def parse_args(argv=None):
    ap = _cli.capture_parser("python -m nlosgr.phasor", "ph.npz",
                             "Phasor-field reconstruction of a confocal or non-confocal capture (the optional field "
                             "laserGridPositions) on a voxel grid.")
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--wavelength", type=float, required=True,
                    help="virtual wavelength in scene units along the whole path (2-4 wall-point spacings or more)")
    ap.add_argument("--cycles", type=float, default=4.0, help="periods inside +-3 sigma of the envelope")
    ap.add_argument("--power", type=int, default=0, choices=range(5), help="weight d^power")
    return _cli.parse(ap, argv)


def main(argv=None):
    a = parse_args(argv)
    dk = _cli.open_capture(a.capture, "phasor")
    out = phasor_capture(dk, a.resolution, a.start, a.end, a.wavelength, cycles=a.cycles, power=a.power)
    # the key names of python -m nlosgr.backproject (density / albedo both hold the magnitude), plus the planes
    _cli.write_volume(a, dk, out, f"wavelength {a.wavelength}, cycles {a.cycles}, power {a.power}",
                      real=out["real"].cpu().numpy(), imag=out["imag"].cpu().numpy())


if __name__ == "__main__":
    main()
