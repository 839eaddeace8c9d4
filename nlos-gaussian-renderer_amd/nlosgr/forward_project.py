"""Forward projection of a voxel grid to the transients of a confocal capture, the adjoint of
nlosgr.backproject, and what it makes possible: checking a volume against the capture, and the least-squares
volume (Landweber iteration).  For voxel centre x and wall point i (include/nlosgr.h, ABI 13):

    d = |x - wall_i|,  u = (d - r0) / dr,  k = floor(u),  f = u - k
    rows_i[j] = sum_x d^power vol(x) ((1-f) [k == j] + f [k+1 == j]),   0 <= j < nr

with d, u, k, f the fp32 values nlosgr_backproject forms, so <A v, h> = <v, A^T h> for powers 0..4.  One HIP
pass (nlosgr_forward_project: a workgroup per wall point and voxel split, 64-bit fixed-point adds into an LDS
row, no float atomics): bitwise repeatable and independent of the split.  A non-finite voxel makes every row
NaN.  Negative powers are the physical falloff; they need r0 >= 2 dr.  No CPU fallback; `project` is the autograd front (its backward is backproject).

A non-confocal capture (`lasers=`: the laser lights another wall point than the one sensed) replaces d by half
the path, g = (|x - laser_i| + |x - wall_i|) / 2, and d^2 by m = |x - laser_i| |x - wall_i| (weight m^(power/2),
-4 the physical 1 / (dl^2 ds^2)), through nlosgr_forward_project_nc; a negative power then leaves out the pairs
closer than `dmin` to the laser or the sensed point.  In either kind of file deltaT is the bin width in HALF-path
units: bin j of a row holds the light whose whole path is 2 (r0 + j c deltaT).

    python -m nlosgr.forward_project CAPTURE.mat --resolution R --start S --end E [--power P] [--iterations N]
        --out lw.npz [--mesh lw.ply --level-frac F]
"""
import ctypes

import numpy as np
import torch

from . import _cli, _lib
from .backproject import _gpu_f32, _lasers_arg, backproject, capture_lasers, fp32_window
from .voxelize import VoxelGrid, front_view


@torch.no_grad()
def box_distance(points, grid):
    """The smallest distance from any of points [n, 3] to the bounding box of the grid's voxel centres (0 when a
    point is inside or on it): a float, one host read."""
    lo = torch.tensor([float(t[0]) for t in grid.tables], device=points.device)
    hi = torch.tensor([float(t[-1]) for t in grid.tables], device=points.device)
    lo, hi = torch.minimum(lo, hi), torch.maximum(lo, hi)
    p = points.double()
    gap = torch.clamp(torch.maximum(lo.double() - p, p - hi.double()), min=0.0)
    return float(gap.square().sum(dim=1).sqrt().min())


@torch.no_grad()
def forward_project(volume, walls, grid, r0, dr, nr, power=0, out=None, accumulate=False, nsplit=0, lasers=None,
                    dmin=None):
    """[nwall, nr] fp32 (the layout data.volume_target returns): the transients of volume [nx, ny, nz] on `grid`
    (voxelize.VoxelGrid) at walls [nwall, 3].  r0: radius of bin 0; dr: bin width; power -4..4: weight d^power.
    out: an [nwall, nr] tensor to write (accumulate=False) or to add this call's rounded sum to
    (accumulate=True: a volume projected as sub-grids or per rank).  nsplit: voxel splits per wall point, 0 = the
    library's choice; the result does not depend on it.  lasers: None for a confocal capture; else the laser
    spots [nwall, 3], or [1, 3] for one spot, of a non-confocal capture whose walls are the sensed points (r0 and
    dr then count half the path, the weight is (|x - laser| |x - wall|)^(power/2)).  dmin (with lasers and a
    negative power only): pairs closer than dmin to their laser spot or sensed point are left out; None takes
    the smallest distance from any of those points to the grid's bounding box (one host read, rounded down to
    fp32) and raises when that is 0.  dmin without lasers raises."""
    lib = _lib.load()
    volume, walls = _gpu_f32(volume, "forward_project"), _gpu_f32(walls, "forward_project")
    if not isinstance(grid, VoxelGrid):
        raise TypeError("nlosgr: grid must be a voxelize.VoxelGrid")
    shape = grid.shape
    if tuple(volume.shape) != shape or walls.dim() != 2 or walls.shape[1] != 3:
        raise ValueError(f"nlosgr: forward_project takes a volume {shape} (the grid's shape) and walls [nwall, 3]")
    dev = volume.device
    if walls.device != dev:
        raise ValueError(f"nlosgr: walls must be on {dev}")
    nwall, nr = int(walls.shape[0]), int(nr)
    if nr < 1:
        raise ValueError("nlosgr: nr must be >= 1")
    if out is None:
        if accumulate:
            raise ValueError("nlosgr: accumulate=True needs the rows to add to (out=)")
        out = torch.empty((nwall, nr), device=dev)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32:
            raise RuntimeError("nlosgr: forward_project needs float32 GPU tensors (no CPU fallback)")
        if tuple(out.shape) != (nwall, nr) or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"nlosgr: out must be a contiguous {(nwall, nr)} tensor on {dev}")
    if not float(dr) > 0:
        raise ValueError("nlosgr: dr must be > 0")
    xs, ys, zs = grid.on(dev)
    vg = _lib.VoxelGrid(shape[0], shape[1], shape[2], _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(zs))
    opt = _lib.ForwardProjectOpts(*fp32_window(r0, dr), int(power), int(bool(accumulate)), int(nsplit))
    if lasers is None:
        if dmin is not None:
            raise ValueError("nlosgr: dmin= belongs to a non-confocal call (lasers=); a confocal one has no use for it")
        nbytes = lib.nlosgr_forward_project_workspace_bytes(nwall, nr, ctypes.byref(vg), ctypes.byref(opt))
    else:
        lasers = _lasers_arg(lasers, walls, "forward_project")
        if int(power) >= 0:
            dmin = 0.0                                   # (ignored by the library)
        elif dmin is None:
            # rounded DOWN to fp32 (the library takes a float): no pair at that very distance is left out
            dmin = box_distance(torch.cat([walls, lasers]), grid) if nwall else 1.0
            f = np.float32(dmin)
            dmin = float(f if float(f) <= dmin else np.nextafter(f, np.float32(0.0)))
            if not dmin > 0:
                raise ValueError("nlosgr: a sensor or laser point lies inside the grid's bounding box, so a negative "
                                 "power has no bound on its weight: pass dmin= (pairs closer than dmin are left out)")
        nl = int(lasers.shape[0])
        nbytes = lib.nlosgr_forward_project_nc_workspace_bytes(nl, nwall, nr, ctypes.byref(vg), ctypes.byref(opt),
                                                               float(dmin))
    if nbytes == 0:
        raise RuntimeError("nlosgr error: " + lib.nlosgr_last_error().decode(errors="replace"))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if lasers is None:
        _lib.check(lib.nlosgr_forward_project(_lib.ptr(volume), _lib.ptr(walls), nwall, nr, ctypes.byref(vg),
                                              ctypes.byref(opt), _lib.ptr(ws), _lib.ptr(out), _lib.stream_handle(dev)))
    else:
        _lib.check(lib.nlosgr_forward_project_nc(_lib.ptr(volume), _lib.ptr(walls), _lib.ptr(lasers), nl, nwall, nr,
                                                 ctypes.byref(vg), ctypes.byref(opt), float(dmin), _lib.ptr(ws),
                                                 _lib.ptr(out), _lib.stream_handle(dev)))
    return out


class _ProjectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, volume, walls, grid, r0, dr, nr, power, lasers):
        ctx.conf = (walls, grid, r0, dr, power, lasers)
        return forward_project(volume, walls, grid, r0, dr, nr, power=power, lasers=lasers)

    @staticmethod
    def backward(ctx, grad_rows):
        walls, grid, r0, dr, power, lasers = ctx.conf
        return (backproject(grad_rows, walls, grid, r0, dr, power=power, lasers=lasers),) + (None,) * 7


def project(volume, walls, grid, r0, dr, nr, power=0, lasers=None):
    """forward_project as a differentiable function of the volume: the forward is forward_project(volume, walls,
    grid, r0, dr, nr, power=, lasers=), the backward with respect to `volume` is backproject of the upstream rows
    with the same arguments (the pair is an exact adjoint).  A volume that requires grad takes powers 0..4 only:
    back-projection has no negative power, so a negative one would have no backward; for the physical falloff
    scale the rows first, as landweber documents."""
    if isinstance(volume, torch.Tensor) and volume.requires_grad and not 0 <= int(power) <= 4:
        raise ValueError("nlosgr: project differentiates through backproject, which takes powers 0..4 only; a volume "
                         f"that requires grad cannot take power {int(power)} (scale the rows by r^q instead)")
    return _ProjectFn.apply(volume, walls, grid, r0, dr, int(nr), int(power), lasers)


def _spacing(t):
    n = int(t.shape[0])
    if n < 2:
        raise ValueError("nlosgr: a voxel volume needs at least two centres per axis")
    return (float(t[-1]) - float(t[0])) / (n - 1)


@torch.no_grad()
def voxel_transient(volume, grid, walls, r, c_deltaT, y):
    """[nwall, nr]: the histogram the Gaussian renderer (no occlusion) produces for a volume holding
    density x albedo (what voxelize returns as `albedo`), on the renderer's radial table r [nr] (geometry.r).
    The renderer's bin is Y^2 c deltaT  integral rho sin(theta) / r^2 dtheta dphi, and dV = r^2 sin(theta) dr dtheta
    dphi, so with dr = (r[-1] - r[0]) / (nr - 1) the table's spacing (a linspace over nr points: not c deltaT) and
    dV the product of the grid's table spacings:

        y^2 (c_deltaT / dr) dV A_-4(volume),   r0 = r[0]

    y: volume_position[1], the renderer's Y."""
    r = torch.as_tensor(r).detach().double().cpu()
    nr = int(r.shape[0])
    if nr < 2:
        raise ValueError("nlosgr: voxel_transient needs a radial table of at least two bins")
    r0, dr = float(r[0]), (float(r[-1]) - float(r[0])) / (nr - 1)
    dv = _spacing(grid.xs) * _spacing(grid.ys) * _spacing(grid.zs)
    rows = forward_project(volume, walls, grid, r0, dr, nr, power=-4)
    return rows.mul_(float(y) ** 2 * (float(c_deltaT) / dr) * dv)


@torch.no_grad()
def operator_norm(walls, grid, r0, dr, nr, power=0, iterations=8, lasers=None):
    """The largest eigenvalue of A^T A (A = forward_project with this window and power 0..4) by power iteration
    from the all-ones volume: a float, one host read at the end.  1 / operator_norm is the Landweber step.
    lasers: as forward_project."""
    walls = _gpu_f32(walls, "operator_norm")
    if not isinstance(grid, VoxelGrid):
        raise TypeError("nlosgr: grid must be a voxelize.VoxelGrid")
    if int(iterations) < 1:
        raise ValueError("nlosgr: iterations must be >= 1")
    v = torch.ones(grid.shape, device=walls.device)
    lam = None
    for _ in range(int(iterations)):
        v = v / v.double().norm().float()
        w = backproject(forward_project(v, walls, grid, r0, dr, nr, power=power, lasers=lasers), walls, grid, r0, dr,
                        power=power, lasers=lasers)
        lam = w.double().norm()
        v = w
    return float(lam)


@torch.no_grad()
def landweber(rows, walls, grid, r0, dr, power=0, iterations=30, nonneg=True, step=None, x0=None, lasers=None):
    """(volume [nx, ny, nz], objective [iterations]): projected gradient on 1/2 |A v - h|^2,
    v <- max(v - step A^T (A v - h), 0) from x0 (zeros by default), step = 1 / operator_norm by default, power
    0..4 (the range of A^T; for the falloff scale the rows by r^q first, as the back-projection's users do).
    objective[n] is 1/2 |A v - h|^2 BEFORE update n, a device tensor (no host read inside the loop).
    lasers: as forward_project (a non-confocal capture)."""
    rows, walls = _gpu_f32(rows, "landweber"), _gpu_f32(walls, "landweber")
    if rows.dim() != 2 or walls.dim() != 2 or walls.shape[1] != 3 or walls.shape[0] != rows.shape[0]:
        raise ValueError("nlosgr: landweber takes rows [nwall, nr] and walls [nwall, 3]")
    if not isinstance(grid, VoxelGrid):
        raise TypeError("nlosgr: grid must be a voxelize.VoxelGrid")
    if not 0 <= int(power) <= 4:
        raise ValueError("nlosgr: landweber takes a power in 0..4 (the range of backproject)")
    nr = int(rows.shape[1])
    if step is None:
        step = 1.0 / operator_norm(walls, grid, r0, dr, nr, power=power, lasers=lasers)
    step = float(step)
    if x0 is None:
        v = torch.zeros(grid.shape, device=rows.device)
    else:
        v = _gpu_f32(x0, "landweber").clone()
        if tuple(v.shape) != grid.shape:
            raise ValueError(f"nlosgr: x0 must have the grid's shape {grid.shape}")
    objective = torch.zeros(int(iterations), dtype=torch.float64, device=rows.device)
    res = torch.empty_like(rows)
    for n in range(int(iterations)):
        forward_project(v, walls, grid, r0, dr, nr, power=power, out=res, lasers=lasers)
        res.sub_(rows)
        objective[n] = 0.5 * res.double().square().sum()
        v.sub_(backproject(res, walls, grid, r0, dr, power=power, lasers=lasers), alpha=step)
        if nonneg:
            v.clamp_(min=0.0)
    return v, objective


@torch.no_grad()
def landweber_capture(data_kwargs, resolution, start, end, power=0, iterations=30):
    """Landweber on the capture in data_kwargs (data.make_data_kwargs) over bins [floor(start), floor(start) +
    end - start) onto VoxelGrid(volume_position, volume_size, resolution), as backproject_capture lays it out; a
    non-confocal capture (data_kwargs["laser_grid_positions"]) with its laser spots.
    Returns {"volume", "objective", "front", "depth", "grid"}."""
    from .data import volume_target
    I1 = int(np.floor(start))
    rows = _gpu_f32(volume_target(data_kwargs, start, int(end - start)), "landweber_capture")
    walls = data_kwargs["camera_grid_positions"].t().contiguous().float()
    vp = data_kwargs["volume_position"]
    grid = VoxelGrid([float(v) for v in vp], float(data_kwargs["volume_size"]), resolution)
    cdt = float(data_kwargs["c"]) * float(data_kwargs["deltaT"])
    vol, obj = landweber(rows, walls, grid, I1 * cdt, cdt, power=power, iterations=iterations,
                         lasers=capture_lasers(data_kwargs))
    front, depth = front_view(vol, grid)
    return {"volume": vol, "objective": obj, "front": front, "depth": depth, "grid": grid}


def parse_args(argv=None):
    ap = _cli.capture_parser("python -m nlosgr.forward_project", "lw.npz",
                             "Least-squares voxel volume of a confocal or non-confocal capture (the optional field "
                             "laserGridPositions): Landweber iteration with the forward projector and the "
                             "back-projection.")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--power", type=int, default=0, choices=range(5), help="weight d^power of the operator")
    ap.add_argument("--iterations", type=int, default=30)
    a = _cli.parse(ap, argv)
    if a.iterations < 1:
        ap.error("--iterations must be >= 1")
    if a.resolution < 2:
        ap.error("--resolution must be >= 2")
    return a


def main(argv=None):
    a = parse_args(argv)
    dk = _cli.open_capture(a.capture, "forward_project")
    out = landweber_capture(dk, a.resolution, a.start, a.end, power=a.power, iterations=a.iterations)
    obj = out["objective"].cpu().numpy()
    _cli.write_volume(a, dk, out, f"power {a.power}, {a.iterations} iterations, objective {obj[0]:.6g} -> {obj[-1]:.6g}",
                      objective=obj)


if __name__ == "__main__":
    main()
