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
import argparse

import numpy as np
import torch

from . import _lib
from .voxelize import MAX_EXTENT, VoxelGrid, front_view

X_ALONG = ("n", "m")


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
    if x_along not in X_ALONG:
        raise ValueError(f"nlosgr: x_along must be one of {X_ALONG}")
    if not float(dr) > 0:
        raise ValueError("nlosgr: dr must be > 0")
    dev = rows.device
    if perm is not None:
        perm = _gpu(perm, torch.int32, "fk_load (perm)")
        if perm.shape != (H * W,) or perm.device != dev:
            raise ValueError(f"nlosgr: perm must be int32 [{H * W}] on {dev}")
        if int(perm.min()) < 0 or int(perm.max()) >= H * W:
            raise ValueError("nlosgr: perm holds a row index outside [0, H W)")
    sm, sn = (W, 1) if x_along == "n" else (1, H)
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


@torch.no_grad()
def fk_capture(data_kwargs, start, end, power=4, amplitude=True, crop=True):
    """f-k migration of the capture in data_kwargs (data.make_data_kwargs, shuffled or not) over bins
    [floor(start), floor(start) + end - start).  crop: keep the voxels inside the capture's volume box
    (volume_position +- volume_size / 2), a contiguous block of the full volume with grid.slice's tables.
    Returns {"volume" [nx,ny,nz], "front", "depth" (voxelize.front_view), "grid"}, the keys of
    backproject_capture.  A non-confocal capture raises NotImplementedError."""
    from .data import is_confocal, volume_target
    if not is_confocal(data_kwargs):
        raise NotImplementedError("nlosgr: f-k migration is confocal only: this capture's laser spots "
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
    vol = fk_migrate(rows, H, W, sx, sz, I1 * cdt, cdt, power=power, amplitude=amplitude,
                     perm=perm.to(rows.device), x_along=x_along)
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
    ap = argparse.ArgumentParser(prog="python -m nlosgr.fk",
                                 description="f-k migration of a confocal capture on its own wall x time lattice "
                                             "(volume, front view, depth).")
    ap.add_argument("capture", help="Zaragoza-format .mat file")
    ap.add_argument("--start", type=int, required=True, help="first time bin")
    ap.add_argument("--end", type=int, required=True, help="one past the last time bin")
    ap.add_argument("--power", type=int, default=4, choices=range(5), help="falloff compensation r^power")
    ap.add_argument("--no-amplitude", action="store_true", help="migrate the compensated rows, not their square root")
    ap.add_argument("--out", default="fk.npz")
    ap.add_argument("--mesh", default=None, help="also write the isosurface as a PLY file")
    ap.add_argument("--level-frac", type=float, default=0.5, help="isosurface level as a fraction of the maximum")
    a = ap.parse_args(argv)
    if a.end <= a.start:
        ap.error("--end must be greater than --start")
    return a


def main(argv=None):
    a = parse_args(argv)
    from .data import make_data_kwargs
    if not torch.cuda.is_available():
        raise RuntimeError("nlosgr: f-k migration needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    dk, *_ = make_data_kwargs(a.capture, dev, shuffle=False)
    out = fk_capture(dk, a.start, a.end, power=a.power, amplitude=not a.no_amplitude)
    grid, vol = out["grid"], out["volume"]
    vp = dk["volume_position"].cpu().numpy().astype(np.float32)
    # the key names of python -m nlosgr.backproject
    np.savez_compressed(a.out, density=vol.cpu().numpy(), albedo=vol.cpu().numpy(), front=out["front"].cpu().numpy(),
                        depth=out["depth"].cpu().numpy(), xs=grid.xs.numpy(), ys=grid.ys.numpy(), zs=grid.zs.numpy(),
                        cam=np.array([vp[0], 0.0, vp[2]], dtype=np.float32))
    print(f"wrote {a.out}: {grid.shape} voxels, {dk['camera_grid_positions'].shape[1]} wall points, bins "
          f"[{a.start}, {a.end}), power {a.power}, {'amplitude' if not a.no_amplitude else 'intensity'}")
    if a.mesh:
        from .mesh import isosurface, write_ply
        level = a.level_frac * float(vol.max())
        mesh = isosurface(vol, grid, level)
        write_ply(a.mesh, mesh)
        print(f"wrote {a.mesh}: level {level:.6g}, {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} triangles")


if __name__ == "__main__":
    main()
