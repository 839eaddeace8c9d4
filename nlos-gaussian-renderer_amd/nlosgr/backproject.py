"""Back-projection of a confocal capture onto a voxel grid: the capture itself in the hidden volume.

Every NLOS reconstruction is compared with it, it is the standard sanity check of a capture file (geometry,
deltaT, the wall order after data_shuffle), and it is a robust initial density (nlosgr.init.
sample_from_backprojection).  For voxel centre x and wall point i with histogram h_i (include/nlosgr.h, ABI 13):

    d = |x - wall_i|,  u = (d - r0) / dr,  k = floor(u),  f = u - k
    out(x) = sum_i d^power ((1-f) h_i[k] + f h_i[k+1])          h_i[j] = 0 outside [0, nr)

r0 is the radius of bin 0 of the rows and dr = c deltaT the bin width, in the units of the renderer's radial
grid.  One HIP pass (nlosgr_backproject: 8^3 bricks, wall points streamed through LDS, fixed summation order, no
atomics): bitwise repeatable, and a sub-grid (VoxelGrid.slice) gives exactly the numbers of the full grid.  The
volume feeds the parts that take any [nx, ny, nz] tensor: voxelize.project / front_view, mesh.isosurface /
write_ply.  Filtered back-projection filters the rows along time first, through the IRF path:

    backproject(irf_apply(rows, time_filter("log", sigma_bins=2.0)), walls, grid, r0, dr)

A non-confocal capture (the laser lights another wall point than the one sensed; `lasers=`) replaces d by half
the path, g = (|x - laser_i| + |x - wall_i|) / 2, and d^2 by m = |x - laser_i| |x - wall_i| (weight m^(power/2)),
through nlosgr_backproject_nc; with lasers == walls that is the confocal result.  In either kind of file deltaT is
the bin width in HALF-path units: bin j of a row holds the light whose whole path is 2 (r0 + j c deltaT).

No CPU fallback, no backward.

    python -m nlosgr.backproject CAPTURE.mat --resolution 128 --start S --end E [--power P]
        [--filter none|laplacian|log] [--sigma-bins B] --out bp.npz [--mesh bp.ply --level-frac F]
"""
import ctypes
import math

import numpy as np
import torch

from . import _cli, _lib
from .irf import IRF, irf_apply
from .voxelize import VoxelGrid, front_view

FILTERS = ("none", "laplacian", "log")


def _gpu_f32(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError(f"nlosgr: {what} needs float32 GPU tensors (no CPU fallback)")
    return t.detach().contiguous()


def _lasers_arg(lasers, walls, what):
    """lasers= of the voxel operators: a float32 [nmeas, 3] or [1, 3] tensor on the walls' device."""
    lasers = _gpu_f32(lasers, what)
    if lasers.dim() != 2 or lasers.shape[1] != 3 or int(lasers.shape[0]) not in (1, int(walls.shape[0])):
        raise ValueError(f"nlosgr: lasers must be [{int(walls.shape[0])}, 3] (one per measurement) or [1, 3]")
    if lasers.device != walls.device:
        raise ValueError(f"nlosgr: lasers must be on {walls.device}")
    return lasers


def capture_lasers(data_kwargs):
    """[nmeas, 3] or [1, 3] laser spots of a capture's data_kwargs (data.make_data_kwargs), or None for a
    confocal capture (no "laser_grid_positions" key)."""
    lasers = data_kwargs.get("laser_grid_positions")
    return None if lasers is None else lasers.t().contiguous().float()


def fp32_window(r0, dr):
    """(r0, inv_dr) as the fp32 values nlosgr_backproject computes with: r0 rounded to fp32 and the fp32
    quotient 1 / dr (a float64 check of a result has to start from these two)."""
    return float(np.float32(r0)), float(np.float32(1.0) / np.float32(dr))


@torch.no_grad()
def backproject(rows, walls, grid, r0, dr, power=0, out=None, accumulate=False, lasers=None):
    """[nx, ny, nz] fp32: the back-projection of rows [nwall, nr] (the layout data.volume_target returns)
    measured at walls [nwall, 3] onto `grid` (voxelize.VoxelGrid).  r0: radius of bin 0; dr: bin width;
    power 0..4: weight d^power (falloff compensation).  out: an [nx, ny, nz] tensor to write (accumulate=False)
    or to add this call's sum to (accumulate=True: a wall back-projected in batches or per rank; one more
    rounding per call, so close to, not bitwise equal to, one call).  lasers: None for a confocal capture;
    else the laser spots [nwall, 3], or [1, 3] for one spot, of a non-confocal capture whose walls are the sensed
    points (r0 and dr then count half the path, the weight is (|x - laser| |x - wall|)^(power/2))."""
    lib = _lib.load()
    rows, walls = _gpu_f32(rows, "backproject"), _gpu_f32(walls, "backproject")
    if rows.dim() != 2 or walls.dim() != 2 or walls.shape[1] != 3 or walls.shape[0] != rows.shape[0]:
        raise ValueError("nlosgr: backproject takes rows [nwall, nr] and walls [nwall, 3]")
    if lasers is not None:
        lasers = _lasers_arg(lasers, walls, "backproject")
    if not isinstance(grid, VoxelGrid):
        raise TypeError("nlosgr: grid must be a voxelize.VoxelGrid")
    dev = rows.device
    shape = grid.shape
    if out is None:
        if accumulate:
            raise ValueError("nlosgr: accumulate=True needs the volume to add to (out=)")
        out = torch.empty(shape, device=dev)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
            raise RuntimeError("nlosgr: backproject needs float32 GPU tensors (no CPU fallback)")
        if tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"nlosgr: out must be a contiguous {shape} tensor on {dev}")
    if not float(dr) > 0:
        raise ValueError("nlosgr: dr must be > 0")
    xs, ys, zs = grid.on(dev)
    vg = _lib.VoxelGrid(shape[0], shape[1], shape[2], _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(zs))
    opt = _lib.BackprojectOpts(*fp32_window(r0, dr), int(power), int(bool(accumulate)))
    if lasers is None:
        _lib.check(lib.nlosgr_backproject(_lib.ptr(rows), _lib.ptr(walls), rows.shape[0], rows.shape[1],
                                          ctypes.byref(vg), ctypes.byref(opt), _lib.ptr(out), _lib.stream_handle(dev)))
    else:
        _lib.check(lib.nlosgr_backproject_nc(_lib.ptr(rows), _lib.ptr(walls), _lib.ptr(lasers), lasers.shape[0],
                                             rows.shape[0], rows.shape[1], ctypes.byref(vg), ctypes.byref(opt),
                                             _lib.ptr(out), _lib.stream_handle(dev)))
    return out


def time_filter(kind, sigma_bins=2.0):
    """The time-axis filter of filtered back-projection as an nlosgr.irf.IRF (apply it with irf_apply):
    "laplacian": minus the second difference, taps [-1, 2, -1], centre 1;
    "log": the same applied to a normalised Gaussian of sigma_bins, truncated at 4 sigma (Laplacian of
    Gaussian: the band-pass that keeps a surface's onset and drops the slowly varying background)."""
    lap = np.array([-1.0, 2.0, -1.0])
    if kind == "laplacian":
        return IRF(lap, 1, 0.0)
    if kind == "log":
        if not sigma_bins > 0:
            raise ValueError("nlosgr: sigma_bins must be > 0")
        n = max(1, int(math.ceil(4.0 * float(sigma_bins))))
        k = np.arange(-n, n + 1, dtype=np.float64)
        g = np.exp(-0.5 * (k / float(sigma_bins)) ** 2)
        return IRF(np.convolve(g / g.sum(), lap), n + 1, 0.0)
    raise ValueError(f"nlosgr: unknown time filter {kind!r} (laplacian, log)")


@torch.no_grad()
def backproject_capture(data_kwargs, resolution, start, end, power=0, filter="log", sigma_bins=2.0, positive=True):
    """Back-projection of the capture in data_kwargs (data.make_data_kwargs: the shuffled wall order is the
    order of both the rows and the wall points) over bins [floor(start), floor(start) + end - start) onto
    VoxelGrid(volume_position, volume_size, resolution).  filter: "none", "laplacian" or "log" (time_filter);
    positive: clamp at zero.  A non-confocal capture (data_kwargs["laser_grid_positions"]) is back-projected with
    its laser spots.  Returns {"volume" [nx,ny,nz], "front", "depth" (voxelize.front_view), "grid"}."""
    from .data import volume_target
    if filter not in FILTERS:
        raise ValueError(f"nlosgr: filter must be one of {FILTERS}")
    I1 = int(np.floor(start))
    rows = volume_target(data_kwargs, start, int(end - start))
    walls = data_kwargs["camera_grid_positions"].t().contiguous().float()
    if filter != "none":
        rows = irf_apply(_gpu_f32(rows, "backproject_capture"), time_filter(filter, sigma_bins))
    vp = data_kwargs["volume_position"]
    grid = VoxelGrid([float(v) for v in vp], float(data_kwargs["volume_size"]), resolution)
    cdt = float(data_kwargs["c"]) * float(data_kwargs["deltaT"])
    vol = backproject(rows, walls, grid, I1 * cdt, cdt, power=power, lasers=capture_lasers(data_kwargs))
    if positive:
        vol.clamp_(min=0.0)
    front, depth = front_view(vol, grid)
    return {"volume": vol, "front": front, "depth": depth, "grid": grid}


def parse_args(argv=None):
    ap = _cli.capture_parser("python -m nlosgr.backproject", "bp.npz",
                             "Back-project a confocal or non-confocal capture (the optional field laserGridPositions) "
                             "onto a voxel grid (volume, front view, depth).")
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--power", type=int, default=0, choices=range(5), help="weight d^power")
    ap.add_argument("--filter", choices=FILTERS, default="log")
    ap.add_argument("--sigma-bins", type=float, default=2.0)
    return _cli.parse(ap, argv)


def main(argv=None):
    a = parse_args(argv)
    dk = _cli.open_capture(a.capture, "backproject")
    out = backproject_capture(dk, a.resolution, a.start, a.end, power=a.power, filter=a.filter, sigma_bins=a.sigma_bins)
    _cli.write_volume(a, dk, out, f"filter {a.filter}, power {a.power}")


if __name__ == "__main__":
    main()
