"""Gaussian initialisation on the GPU: random init and space carving with the
reference's names, arguments and random-number calls (gaussian_model/gaussian_utils.py:8-166).

The reference's space carving loops over every wall point in Python, one torch pass over all
voxels each (gaussian_utils.py:88-99). Here the vote is one HIP launch (`nlosgr_carve_votes`,
lane = voxel, wall points streamed through LDS), and the first-bounce detection
(`detect_first_bounces`, :38-49, a double Python loop over the wall) is one vectorised torch pass.
Meshing (`exact_mesh_samping=True`) needs open3d/trimesh, which the reference imports and this
image lacks: it raises.

`sample_from_backprojection` is an addition without a counterpart in the reference: it draws the initial
points from the capture's back-projection (nlosgr.backproject) instead of a carved set, so it does not depend
on a first-bounce threshold and works on captures with a dark-count floor and shot noise.  It also takes a
non-confocal capture (data_kwargs["laser_grid_positions"]: the laser spot differs from the sensed one), which
the carving cannot; in such a file deltaT is the bin width in half-path units, as in a confocal one.  With
method="fk" the volume drawn from is the capture's f-k migration (nlosgr.fk), a few passes over the capture in
place of the full back-projection.  `sample_from_volume` is its drawing half alone, for a volume that is already
there (the "volume" and "grid" of nlosgr.lct.lct_capture or of any other *_capture).
"""
import numpy as np
import torch

from . import _lib


def init_rand_points(args, data_kwargs, margin=0.1, rho_scale=0.1, device="cuda"):
    """gaussian_utils.py:8-32: uniform samples in the volume box shrunk by `margin`, rho ~ U(0, rho_scale)
    (numpy global generator, same calls and order as the reference)."""
    n = args.init_gaussian_num
    rho = np.random.rand(n, 1) * rho_scale
    pmin, pmax = data_kwargs["pmin"], data_kwargs["pmax"]
    pmin_c, pmax_c = pmin[:3].cpu().numpy(), pmax[:3].cpu().numpy()
    samples = np.random.rand(n, 3)
    lo = pmin_c + np.abs(pmin_c * margin)
    hi = pmax_c - np.abs(pmax_c * margin)
    return samples * (hi[None] - lo[None]) + lo[None], rho


@torch.no_grad()
def detect_first_bounces(transient, threshold=1e-5):
    """gaussian_utils.py:38-49: per wall pixel (y, x) the first bin b >= 1 with
    transient[b] - transient[b-1] > threshold, 0 if none or if the histogram sums to 0.
    transient [T, H, W] (numpy or torch); returns the same kind, [H, W] float."""
    is_np = isinstance(transient, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(transient)) if is_np else transient
    jump = (t[1:] - t[:-1]) > threshold                          # [T-1, H, W], fp32 differences as in numpy
    has = jump.any(dim=0) & (t.sum(dim=0, dtype=torch.float64) != 0)
    first = jump.to(torch.int8).argmax(dim=0) + 1                 # first True (argmax of a 0/1 array)
    out = torch.where(has, first, torch.zeros_like(first)).to(torch.float64 if is_np else torch.float32)
    return out.numpy() if is_np else out


def carve_votes(coords, walls, radius):
    """votes [N] int32: number of first-bounce spheres (walls [M,3], radius [M]) each voxel of
    coords [N,3] lies outside of (radius <= 0 skipped) — one nlosgr_carve_votes launch."""
    lib = _lib.load()
    for t in (coords, walls, radius):
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError("nlosgr: carve_votes needs float32 GPU tensors (no CPU fallback)")
    coords, walls, radius = coords.contiguous(), walls.contiguous(), radius.contiguous()
    votes = torch.empty(coords.shape[0], dtype=torch.int32, device=coords.device)
    _lib.check(lib.nlosgr_carve_votes(_lib.ptr(coords), coords.shape[0], _lib.ptr(walls), _lib.ptr(radius),
                                      walls.shape[0], _lib.ptr(votes), _lib.stream_handle(coords.device)))
    return votes


@torch.no_grad()
def space_carving(args, data_kwargs):
    """gaussian_utils.py:52-122: voxels of a carving_volume_size^3 grid over the hidden volume that lie
    outside more than space_carving_ratio x max first-bounce spheres; returns their world coordinates
    [Nt, 3] (voxel order of the reference's meshgrid('ij'))."""
    start, threshold = 0, 1e-5      # the reference's only configured scene (zaragoza_bunny, :70-74)
    grid = data_kwargs["camera_grid_positions"]                       # [3, MN]
    device = grid.device
    volume_position = data_kwargs["volume_position"]
    volume_size = data_kwargs["volume_size"]
    c, deltaT = data_kwargs["c"], data_kwargs["deltaT"]
    walls = (grid - volume_position[:, None]).t().contiguous().float()   # shifted origin, [MN, 3]
    nlos = data_kwargs["nlos_data"]
    radii = start + detect_first_bounces(nlos[start:].float(), threshold=threshold).double()
    radii = (radii * c * deltaT).reshape(-1)
    n = args.carving_volume_size
    axis = np.linspace(-volume_size / 2, volume_size / 2, n)
    coords = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    coords = torch.from_numpy(coords.astype(np.float32)).to(device)
    # the reference compares fp32 distances with the python-float radius cast to fp32
    votes = carve_votes(coords, walls, radii.to(device=device, dtype=torch.float32))
    thr = votes.max().item() * args.space_carving_ratio
    keep = votes > thr
    return coords[torch.nonzero(keep, as_tuple=True)[0]] + volume_position[None]


def sample_from_feasible_space_jittering(args, data_kwargs, margin=0.1, rho_scale=0.1, device="cuda",
                                         exact_mesh_samping=False):
    """gaussian_utils.py:124-166: init_gaussian_num carved voxels drawn with torch.randint and jittered
    by up to half a grid spacing (torch.rand_like), rho ~ U(0, rho_scale) (numpy) — same calls."""
    n = args.init_gaussian_num
    rho = np.random.rand(n, 1) * rho_scale
    coords2 = space_carving(args, data_kwargs)
    if exact_mesh_samping:
        raise NotImplementedError("nlosgr: mesh-based sampling needs open3d / trimesh (absent)")
    pmin, pmax = data_kwargs["pmin"], data_kwargs["pmax"]
    spacing = ((pmax - pmin) / (args.carving_volume_size - 1))[:3]
    half = spacing / 2.0
    idx = torch.randint(0, coords2.shape[0], (n,), device=coords2.device)
    base = coords2[idx]
    return base + (torch.rand_like(base) - 0.5) * 2 * half[None], rho


@torch.no_grad()
def sample_from_backprojection(args, data_kwargs, margin=0.1, rho_scale=0.1, device="cuda", start=None, end=None,
                               power=0, filter="log", gamma=1.0, wavelength=None, cycles=4.0,
                               method="backprojection", fk_power=4):
    """Data-driven initialisation that does not rest on a first-bounce threshold: init_gaussian_num voxels of
    the capture's back-projection (nlosgr.backproject.backproject_capture on a carving_volume_size^3 grid,
    clamped at 0) drawn with torch.multinomial in proportion to volume**gamma, with replacement, and jittered
    by up to half a grid spacing as the carving sampler does; rho ~ U(0, rho_scale) (numpy), as the other
    two.  Voxels outside the volume box shrunk by `margin` (the rule of init_rand_points) are not drawn.
    start / end default to args.start / args.end, or the whole capture.  wavelength: when given, the volume
    drawn from is the phasor-field magnitude (nlosgr.phasor.phasor_capture with this wavelength and `cycles`;
    `filter` is then unused) instead of the filtered back-projection.  method="fk": the volume drawn from is the
    capture's f-k migration cropped to the volume box (nlosgr.fk.fk_capture: a few passes over the capture instead
    of a full back-projection; confocal captures with a lattice wall only; carving_volume_size, filter and
    wavelength are unused), and the jitter is half that volume's own spacing per axis (wall spacing, bin width),
    not the carving cube's; its falloff weight is fk_power (`power` belongs to the back-projection and the phasor
    field).  method="rsd": the volume drawn from is the fast phasor field (nlosgr.rsd.rsd_capture with `wavelength`,
    which it needs, `cycles` and `power`: the wall's lattice x carving_volume_size depth planes, cropped to the
    volume box; a confocal capture or one laser spot, on a lattice wall), and the jitter is again half that
    volume's own spacing per axis.
    Returns (points [n,3], rho [n,1])."""
    from .backproject import backproject_capture
    if method not in ("backprojection", "fk", "rsd"):
        raise ValueError("nlosgr: method must be 'backprojection', 'fk' or 'rsd'")
    if method == "rsd" and wavelength is None:
        raise ValueError("nlosgr: method='rsd' is the phasor field: it needs wavelength=")
    n = args.init_gaussian_num
    rho = np.random.rand(n, 1) * rho_scale
    if start is None:
        start = getattr(args, "start", 0)
    if end is None:
        end = getattr(args, "end", None)
        if end is None:
            end = data_kwargs["nlos_data"].shape[0]
    if method == "fk":
        from .fk import fk_capture
        out = fk_capture(data_kwargs, start, end, power=fk_power)
    elif method == "rsd":
        from .rsd import rsd_capture
        out = rsd_capture(data_kwargs, args.carving_volume_size, start, end, wavelength, cycles=cycles, power=power)
    else:
        res = args.carving_volume_size
        if wavelength is None:
            out = backproject_capture(data_kwargs, res, start, end, power=power, filter=filter, positive=True)
        else:
            from .phasor import phasor_capture
            out = phasor_capture(data_kwargs, res, start, end, wavelength, cycles=cycles, power=power)
    vol, grid = out["volume"], out["grid"]
    dev = vol.device
    pmin, pmax = data_kwargs["pmin"][:3].to(dev), data_kwargs["pmax"][:3].to(dev)
    lo = pmin + (pmin * margin).abs()
    hi = pmax - (pmax * margin).abs()
    xs, ys, zs = grid.on(dev)
    inside = (((xs >= lo[0]) & (xs <= hi[0]))[:, None, None] & ((ys >= lo[1]) & (ys <= hi[1]))[None, :, None]
              & ((zs >= lo[2]) & (zs <= hi[2]))[None, None, :])
    w = torch.where(inside, vol, torch.zeros_like(vol)).reshape(-1).double()
    if gamma != 1.0:
        w = w ** gamma
    if not bool(torch.isfinite(w).all()) or not float(w.sum()) > 0:
        raise RuntimeError("nlosgr: the back-projection is zero (or not finite) inside the margin box: nothing to "
                           "sample from (check start / end, the filter and the capture's geometry)")
    idx = torch.multinomial(w / w.sum(), n, replacement=True)
    ny, nz = vol.shape[1], vol.shape[2]
    base = torch.stack((xs[idx // (ny * nz)], ys[(idx // nz) % ny], zs[idx % nz]), dim=1)
    if method in ("fk", "rsd"):
        half = torch.stack([(t[-1] - t[0]) / max(t.numel() - 1, 1) for t in (xs, ys, zs)]) / 2.0
    else:
        half = ((pmax - pmin) / (res - 1)) / 2.0
    return base + (torch.rand_like(base) - 0.5) * 2 * half[None], rho


@torch.no_grad()
def sample_from_volume(args, data_kwargs, volume, grid, margin=0.1, rho_scale=0.1, gamma=1.0):
    """The drawing half of sample_from_backprojection for a volume that is already there: init_gaussian_num voxels
    of `volume` [nx, ny, nz] on `grid` (a voxelize.VoxelGrid) drawn with torch.multinomial in proportion to
    max(volume, 0)**gamma, with replacement, and jittered by up to half the grid's own spacing per axis
    ((last - first) / (n - 1) of each table); rho ~ U(0, rho_scale) (numpy).  Voxels outside the volume box shrunk
    by `margin` are not drawn.  It takes the "volume" and "grid" of any *_capture result:
        out = lct_capture(dk, start, end);  sample_from_volume(args, dk, **{k: out[k] for k in ("volume", "grid")})
    The generators are called as sample_from_backprojection calls them: numpy for rho first, then torch.multinomial
    and torch.rand_like on the volume's device.  Returns (points [n,3], rho [n,1])."""
    n = args.init_gaussian_num
    rho = np.random.rand(n, 1) * rho_scale
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3 or tuple(volume.shape) != tuple(grid.shape):
        raise ValueError(f"nlosgr: volume must be a tensor of the grid's shape {tuple(grid.shape)}")
    vol = volume.detach()
    dev = vol.device
    pmin, pmax = data_kwargs["pmin"][:3].to(dev), data_kwargs["pmax"][:3].to(dev)
    lo = pmin + (pmin * margin).abs()
    hi = pmax - (pmax * margin).abs()
    xs, ys, zs = grid.on(dev)
    inside = (((xs >= lo[0]) & (xs <= hi[0]))[:, None, None] & ((ys >= lo[1]) & (ys <= hi[1]))[None, :, None]
              & ((zs >= lo[2]) & (zs <= hi[2]))[None, None, :])
    w = torch.where(inside, vol, torch.zeros_like(vol)).clamp_min(0).reshape(-1).double()
    if gamma != 1.0:
        w = w ** gamma
    if not bool(torch.isfinite(w).all()) or not float(w.sum()) > 0:
        raise RuntimeError("nlosgr: the volume is zero (or not finite) inside the margin box: nothing to sample from")
    idx = torch.multinomial(w / w.sum(), n, replacement=True)
    ny, nz = vol.shape[1], vol.shape[2]
    base = torch.stack((xs[idx // (ny * nz)], ys[(idx // nz) % ny], zs[idx % nz]), dim=1)
    half = torch.stack([(t[-1] - t[0]) / max(t.numel() - 1, 1) for t in (xs, ys, zs)]) / 2.0
    return base + (torch.rand_like(base) - 0.5) * 2 * half[None], rho
