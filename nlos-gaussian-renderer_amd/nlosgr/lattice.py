"""The wall's lattice, shared by the reconstructions that live on it (nlosgr.fk, nlosgr.rsd, nlosgr.lct): how a
capture's wall becomes a uniform H x W lattice (wall_lattice), how lattice point (m, n) finds its row (lattice_rows), the
prologue and the crop of the three *_capture functions (capture_lattice, capture_result), the grid of a volume on the
lattice (fk_grid) and the argument checks the three modules' stage functions share.

Lattice point (m, n) is measured at (xs[n], y0, zs[m]); its row is rows[perm[v]] (perm None: rows[v]) with
v = m W + n (x_along="n") or v = n H + m (x_along="m").
"""
from typing import NamedTuple

import numpy as np
import torch

from .voxelize import MAX_EXTENT, VoxelGrid, front_view

X_ALONG = ("n", "m")


def _f32(v):
    return float(np.float32(v))


def _gpu(t, dtype, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
        raise RuntimeError(f"nlosgr: {what} needs {str(dtype).replace('torch.', '')} GPU tensors (no CPU fallback)")
    return t.detach().contiguous()


def _extents(H, W, nr):
    H, W, nr = int(H), int(W), int(nr)
    if not (1 <= H <= MAX_EXTENT and 1 <= W <= MAX_EXTENT and 1 <= nr <= MAX_EXTENT):
        raise ValueError(f"nlosgr: f-k extents H, W, nr must be in 1..{MAX_EXTENT}")
    return H, W, nr


def _work(out, shape, dev, what):
    """A complex64 work array [2H, 2W, 2nr]: `out` checked, or a new one."""
    if out is None:
        return torch.empty(shape, dtype=torch.complex64, device=dev)
    if isinstance(out, torch.Tensor) and not out.is_contiguous():     # (a copy would be filled, not the caller's)
        raise ValueError(f"nlosgr: out must be a contiguous complex64 {tuple(shape)} tensor on {dev}")
    out = _gpu(out, torch.complex64, what)
    if tuple(out.shape) != tuple(shape) or out.device != dev:
        raise ValueError(f"nlosgr: out must be a contiguous complex64 {tuple(shape)} tensor on {dev}")
    return out


def lattice_rows(perm, x_along, H, W, dev, what):
    """(perm checked, stride_m, stride_n): how lattice point (m, n) finds its row.  The kernels clamp what perm
    names, so a bad entry could only pick a wrong row; this check (one perm.min() and one perm.max() read back)
    turns it into an error."""
    if x_along not in X_ALONG:
        raise ValueError(f"nlosgr: x_along must be one of {X_ALONG}")
    if perm is not None:
        perm = _gpu(perm, torch.int32, f"{what} (perm)")
        if perm.shape != (H * W,) or perm.device != dev:
            raise ValueError(f"nlosgr: perm must be int32 [{H * W}] on {dev}")
        if int(perm.min()) < 0 or int(perm.max()) >= H * W:
            raise ValueError("nlosgr: perm holds a row index outside [0, H W)")
    return (perm,) + ((W, 1) if x_along == "n" else (1, H))


def wall_lattice(data_kwargs):
    """(H, W, xs, zs, y0, perm, x_along) of the capture in data_kwargs (data.make_data_kwargs; CPU or GPU tensors):
    its wall as a uniform H x W lattice on a plane y = y0, x = xs[n] (fp32 [W]) and z = zs[m] (fp32 [H]), with
    perm (int32 [H W], on the capture's device) the inverse of data_kwargs["index"]: the column of nlos_data that
    holds unshuffled wall point v, so shuffled and unshuffled captures give the same lattice.  x_along: "n" when x
    runs along the last axis of nlos_data [T, M, N] (then H = M, W = N), "m" when it runs along M (H = N, W = M).
    Raises ValueError when the unshuffled points are not such a lattice to 1e-4 of the spacing, or when a
    coordinate decreases.  An axis of one point takes the other axis's spacing."""
    _, M, N = data_kwargs["nlos_data"].shape
    M, N = int(M), int(N)
    pos = data_kwargs["camera_grid_positions"]
    index = data_kwargs["index"]
    if tuple(pos.shape) != (3, M * N) or index.numel() != M * N:
        raise ValueError(f"nlosgr: camera_grid_positions must be [3, {M * N}] and index [{M * N}]")
    idx = index.reshape(-1).long()
    if not torch.equal(idx.sort().values, torch.arange(M * N, device=idx.device)):
        raise ValueError("nlosgr: index is not a permutation of the wall points")
    perm = torch.empty_like(idx)
    perm[idx] = torch.arange(M * N, device=idx.device)
    p = pos.detach().double()[:, perm].cpu().numpy().reshape(3, M, N)
    x, y, z = p
    span = lambda a, axis: float(np.abs(np.diff(a, axis=axis)).max()) if a.shape[axis] > 1 else 0.0
    # the coordinate that moves along N tells the orientation (a 1 x N wall: whichever of x, z moves)
    if span(x, 1) >= span(z, 1) and span(z, 0) >= span(x, 0):
        x_along, xs, zs = "n", x[0, :], z[:, 0]
        X, Z = np.broadcast_to(xs[None, :], (M, N)), np.broadcast_to(zs[:, None], (M, N))
    else:
        x_along, xs, zs = "m", x[:, 0], z[0, :]
        X, Z = np.broadcast_to(xs[:, None], (M, N)), np.broadcast_to(zs[None, :], (M, N))
    W, H = len(xs), len(zs)
    if W == 1 and H == 1:
        raise ValueError("nlosgr: a wall of one point has no lattice spacing")
    steps = [(t[-1] - t[0]) / (len(t) - 1) for t in (xs, zs) if len(t) > 1]
    if min(steps) <= 0:
        raise ValueError("nlosgr: a wall coordinate decreases along its axis (or does not move): not a lattice "
                         "f-k migration can use")
    sx = steps[0] if W > 1 else steps[-1]
    sz = steps[-1] if H > 1 else steps[0]
    tol = 1e-4 * min(sx, sz)
    ideal_x, ideal_z = xs[0] + sx * np.arange(W), zs[0] + sz * np.arange(H)
    y0 = float(y.reshape(-1)[0])
    if (np.abs(xs - ideal_x).max() > tol or np.abs(zs - ideal_z).max() > tol or np.abs(x - X).max() > tol
            or np.abs(z - Z).max() > tol or np.abs(y - y0).max() > tol):
        raise ValueError("nlosgr: the wall points are not a uniform lattice on a plane y = const (to 1e-4 of the "
                         "spacing): f-k migration needs one")
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return H, W, f32(xs), f32(zs), y0, perm.to(torch.int32), x_along


def lattice_spacing(t, other=None):
    """The uniform spacing of a lattice table (float64 from its end points); a table of one point takes `other`."""
    if len(t) > 1:
        return float((t[-1].double() - t[0].double()) / (len(t) - 1))
    if other is None:
        raise ValueError("nlosgr: a lattice axis of one point has no spacing")
    return float(other)


def fk_grid(xs, zs, y0, r0, dr, nr):
    """The VoxelGrid of an f-k volume [W, nr, H]: xs and zs are the wall lattice's own tables and ys[j] = y0 + r0 +
    j dr (built in double, rounded to fp32).  nr, H, W <= 1024 (VoxelGrid.MAX_EXTENT), else ValueError."""
    f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64).astype(np.float32)).reshape(-1)
    ys = float(y0) + float(r0) + float(dr) * np.arange(int(nr), dtype=np.float64)
    return VoxelGrid(tables=(f32(xs), f32(ys), f32(zs)))


def _inside(t, lo, hi):
    """(start, stop) of the contiguous run of table entries within [lo, hi] (tables ascend)."""
    ok = np.nonzero((t >= lo) & (t <= hi))[0]
    if ok.size == 0:
        raise ValueError("nlosgr: no voxel of the f-k volume lies inside the capture's volume box")
    return int(ok[0]), int(ok[-1]) + 1


class CaptureLattice(NamedTuple):
    """A capture on its wall lattice (capture_lattice)."""
    rows: torch.Tensor     # [H W, nr], the capture's own row order
    H: int
    W: int
    xs: torch.Tensor       # fp32 [W], CPU
    zs: torch.Tensor       # fp32 [H], CPU
    y0: float
    perm: torch.Tensor     # int32 [H W] on the rows' device
    x_along: str
    sx: float
    sz: float
    r0: float              # radius of bin 0
    dr: float              # bin width
    nr: int


def capture_lattice(data_kwargs, start, end, extents=True):
    """The capture in data_kwargs (data.make_data_kwargs, shuffled or not) over bins [floor(start), floor(start) +
    end - start) on its wall lattice, a CaptureLattice: wall_lattice's fields, the rows, the window r0 = floor(start)
    c deltaT, dr = c deltaT, and the spacings (an axis of one point takes the other's).  extents: refuse H, W or nr
    beyond 1024, for a volume [W, nr, H] on the lattice itself (nlosgr.rsd's depths are its own: it passes False).
    Whether the capture is confocal is the caller's question."""
    from .data import volume_target
    I1 = int(np.floor(start))
    nr = int(end - start)
    H, W, xs, zs, y0, perm, x_along = wall_lattice(data_kwargs)
    if extents:
        _extents(H, W, nr)
    rows = volume_target(data_kwargs, start, nr)
    cdt = float(data_kwargs["c"]) * float(data_kwargs["deltaT"])
    sx = lattice_spacing(xs, None if len(xs) > 1 else lattice_spacing(zs))
    sz = lattice_spacing(zs, sx)
    return CaptureLattice(rows, H, W, xs, zs, y0, perm.to(rows.device), x_along, sx, sz, I1 * cdt, cdt, nr)


def confocal_lattice(data_kwargs, start, end, what):
    """capture_lattice for the operators that are confocal only; `what` names the operator in the refusal."""
    from .data import is_confocal
    if not is_confocal(data_kwargs):
        raise NotImplementedError(f"nlosgr: {what} is confocal only: this capture's laser spots "
                                  "(laser_grid_positions) differ from its sensed points.  Use nlosgr.phasor (or "
                                  "nlosgr.backproject), which take the laser spots")
    return capture_lattice(data_kwargs, start, end)


def capture_result(data_kwargs, grid, vol, crop, axes=(0, 1, 2), **more):
    """The dictionary a *_capture function returns: {"volume", "front", "depth" (voxelize.front_view), "grid"} and
    the tensors in `more` under their names.  crop: cut the grid along `axes` (0: x, 1: y, 2: z) to the capture's
    volume box (volume_position +- volume_size / 2), the contiguous block of its tables inside it, and take the same
    block of every tensor; the other axes are kept whole."""
    if crop:
        vp = [float(v) for v in data_kwargs["volume_position"]]
        h = float(data_kwargs["volume_size"]) / 2
        runs = [_inside(grid.tables[k].numpy(), vp[k] - h, vp[k] + h) if k in axes else None for k in range(3)]
        cut = tuple(slice(None) if r is None else slice(*r) for r in runs)
        vol, more = vol[cut].contiguous(), {k: v[cut].contiguous() for k, v in more.items()}
        grid = grid.slice(*runs)
    front, depth = front_view(vol, grid)
    return {"volume": vol, **more, "front": front, "depth": depth, "grid": grid}
