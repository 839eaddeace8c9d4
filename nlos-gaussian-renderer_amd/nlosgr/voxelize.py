"""Reconstruction output: the trained Gaussians on a regular voxel grid, with projection maps.

The reference's evaluation() calls gaussian2volume (main.py:374-387, nlos_helpers.py:40-69), which evaluates
estimate_rho_w(out_separately=True) at the spherical samples of the central wall point; its per-sample
"density" there is a flattened [Ng * Na] per-Gaussian tensor, which means nothing on a grid.  What is
implemented here are the NO-OCCLUSION definitions, the two sums estimate_rho_w_no_occlusion(
out_separately=True) returns (gaussian_model/gaussian_model.py:346-364), at every voxel centre x:

    density(x)        = sum_g sigma_g pdf_g(x)
    albedo_density(x) = sum_g sigma_g rho_g(cam) pdf_g(x),    rho_g(cam) = max(0, 0.5 + SH_g(dir(mu_g - cam)))

with preset, scaling_modifier, sh_degree and cutoff meaning exactly what they mean for the renderer
(pdf_g = 0 where the Mahalanobis distance exceeds `cutoff`; dense when cutoff <= 0).  One HIP pass
(nlosgr_voxelize: two-level box culling, ordered LDS batches) replaces the dense [Ng, Nvox] torch
broadcast; every voxel's sum runs in ascending Gaussian order, so the result is bitwise repeatable and a
sub-grid (VoxelGrid.slice) gives exactly the numbers of the full grid.  No CPU fallback.

The backward is nlosgr_voxelize_bwd (voxelize_backward; voxelize_params is the torch.autograd front of the
pair): one wave per Gaussian sums the upstream over the Gaussian's own support, the forward's by construction,
without atomics, so a Gaussian's gradient rows do not depend on the other Gaussians or their order.

    python -m nlosgr.voxelize CKPT --resolution 256 --cutoff 3 --volume-position x y z --volume-size s --out recon.npz
"""
import argparse

import numpy as np
import torch

from . import _lib
from .model import features_flat

MAX_EXTENT = 1024


class VoxelGrid:
    """Regular grid of voxel centres.  VoxelGrid(volume_position, volume_size, resolution) spans the cube
    [position - size/2, position + size/2] with `resolution` centres per axis; VoxelGrid(axes=((lo, hi, n),
    ...)) gives each axis explicitly.  Coordinates are linspace(lo, hi, n), end points included, built in
    double and rounded to fp32 as space_carving builds its grid (gaussian_utils.py:91-93); voxel (ix, iy,
    iz) is stored at (ix*ny + iy)*nz + iz (meshgrid 'ij')."""

    def __init__(self, volume_position=None, volume_size=None, resolution=None, axes=None, tables=None):
        if tables is not None:
            self.tables = tuple(tables)
        else:
            if axes is None:
                if volume_position is None or volume_size is None or resolution is None:
                    raise ValueError("nlosgr: VoxelGrid needs (volume_position, volume_size, resolution) or axes")
                pos = [float(v) for v in volume_position]
                res = (resolution,) * 3 if np.isscalar(resolution) else tuple(resolution)
                h = float(volume_size) / 2
                axes = tuple((p - h, p + h, int(n)) for p, n in zip(pos, res))
            if len(axes) != 3:
                raise ValueError("nlosgr: VoxelGrid axes must be three (lo, hi, n) triples")
            self.tables = tuple(torch.from_numpy(np.linspace(float(lo), float(hi), int(n)).astype(np.float32))
                                for lo, hi, n in axes)
        for t in self.tables:
            if t.dim() != 1 or not 1 <= t.shape[0] <= MAX_EXTENT:
                raise ValueError(f"nlosgr: voxel grid extents must be in 1..{MAX_EXTENT}")
        self._dev = {}

    xs = property(lambda self: self.tables[0])
    ys = property(lambda self: self.tables[1])
    zs = property(lambda self: self.tables[2])

    @property
    def shape(self):
        return tuple(int(t.shape[0]) for t in self.tables)

    def slice(self, ix=None, iy=None, iz=None):
        """Sub-grid of index ranges (start, stop) per axis (None keeps the axis); it shares the parent's
        table values, so voxelize() on it returns exactly that block of the parent's result."""
        out = []
        for t, r in zip(self.tables, (ix, iy, iz)):
            out.append(t if r is None else t[int(r[0]):int(r[1])])
        return VoxelGrid(tables=out)

    def on(self, device):
        """The three tables as contiguous fp32 tensors on `device` (cached)."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(device).contiguous() for t in self.tables)
        return self._dev[key]

    def coords(self):
        """[nx, ny, nz, 3] voxel centres (CPU, meshgrid 'ij')."""
        return torch.stack(torch.meshgrid(*self.tables, indexing="ij"), dim=-1)


def _gpu_f32(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError(f"nlosgr: {what} needs float32 GPU tensors (no CPU fallback)")
    return t.detach().contiguous()


@torch.no_grad()
def voxelize(model, grid, cam, preset="cuda", cutoff=3.0, scaling_modifier=1.0, sh_degree=None,
             want_density=True, want_albedo=True):
    """(density, albedo_density), each [nx, ny, nz] fp32 on the model's device (None when not wanted): the
    no-occlusion sums of the module docstring for the Gaussians of `model` (reference attribute names),
    SH albedo viewed from `cam` [3].  One nlosgr_voxelize launch sequence on the current stream."""
    lib = _lib.load()
    mu, scaling, rotation, opacity, feats = [_gpu_f32(t, "voxelize") for t in
                                             (model._mu, model._scaling, model._rotation, model._opacity,
                                              features_flat(model))]
    cam = _gpu_f32(cam, "voxelize").reshape(-1)
    if cam.numel() != 3:
        raise ValueError("nlosgr: cam must have 3 elements")
    dev = mu.device
    ng = mu.shape[0]
    if mu.shape != (ng, 3) or scaling.shape != (ng, 3) or rotation.shape != (ng, 4) or opacity.numel() != ng:
        raise ValueError("nlosgr: mu/scaling must be [Ng,3], rotation [Ng,4], opacity [Ng]")
    deg = int(model.active_sh_degree if sh_degree is None else sh_degree)
    g = _lib.Gaussians(ng, feats.shape[1], deg, _lib.PRESETS[preset], float(scaling_modifier), _lib.ptr(mu),
                       _lib.ptr(scaling), _lib.ptr(rotation), _lib.ptr(opacity), _lib.ptr(feats))
    xs, ys, zs = grid.on(dev)
    nx, ny, nz = grid.shape
    vg = _lib.VoxelGrid(nx, ny, nz, _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(zs))
    opt = _lib.Options(_lib.MODE_NOOCL, float(cutoff), 0.0, 1.0, 0, 0, 0, _lib.SELECT_SUPPORT, 0, 0)
    nbytes = lib.nlosgr_voxel_workspace_bytes(g, vg, opt)
    if nbytes == 0:
        _lib.check(1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dens = torch.empty(nx, ny, nz, device=dev) if want_density else None
    alb = torch.empty(nx, ny, nz, device=dev) if want_albedo else None
    _lib.check(lib.nlosgr_voxelize(g, vg, _lib.ptr(cam), opt, _lib.ptr(ws), _lib.ptr(dens), _lib.ptr(alb),
                                   _lib.stream_handle(dev)))
    return dens, alb


@torch.no_grad()
def voxelize_backward(model, grid, cam, grad_density=None, grad_albedo=None, preset="cuda", cutoff=3.0,
                      scaling_modifier=1.0, sh_degree=None):
    """(d_mu [ng,3], d_scaling [ng,3], d_rotation [ng,4], d_opacity [ng], d_features [ng,K]), the tuple layout of
    render_backward: the gradients of L with respect to the raw parameters of `model`, given grad_density =
    dL/d density and grad_albedo = dL/d albedo_density, each [nx, ny, nz] or None, for the volumes voxelize
    returns under the same arguments.  One nlosgr_voxelize_bwd launch sequence on the current stream; both
    upstreams None gives zeros."""
    lib = _lib.load()
    mu, scaling, rotation, opacity, feats = [_gpu_f32(t, "voxelize_backward") for t in
                                             (model._mu, model._scaling, model._rotation, model._opacity,
                                              features_flat(model))]
    cam = _gpu_f32(cam, "voxelize_backward").reshape(-1)
    if cam.numel() != 3:
        raise ValueError("nlosgr: cam must have 3 elements")
    dev = mu.device
    ng = mu.shape[0]
    if mu.shape != (ng, 3) or scaling.shape != (ng, 3) or rotation.shape != (ng, 4) or opacity.numel() != ng:
        raise ValueError("nlosgr: mu/scaling must be [Ng,3], rotation [Ng,4], opacity [Ng]")
    nx, ny, nz = grid.shape
    ups = []
    for t in (grad_density, grad_albedo):
        if t is not None:
            t = _gpu_f32(t, "voxelize_backward")
            if tuple(t.shape) != (nx, ny, nz) or t.device != dev:
                raise ValueError(f"nlosgr: an upstream gradient must be a {(nx, ny, nz)} tensor on {dev}")
        ups.append(t)
    deg = int(model.active_sh_degree if sh_degree is None else sh_degree)
    g = _lib.Gaussians(ng, feats.shape[1], deg, _lib.PRESETS[preset], float(scaling_modifier), _lib.ptr(mu),
                       _lib.ptr(scaling), _lib.ptr(rotation), _lib.ptr(opacity), _lib.ptr(feats))
    xs, ys, zs = grid.on(dev)
    vg = _lib.VoxelGrid(nx, ny, nz, _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(zs))
    opt = _lib.Options(_lib.MODE_NOOCL, float(cutoff), 0.0, 1.0, 0, 0, 0, _lib.SELECT_SUPPORT, 0, 0)
    nbytes = lib.nlosgr_voxel_bwd_workspace_bytes(g, vg, opt)
    if nbytes == 0:
        _lib.check(1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    outs = (torch.empty_like(mu), torch.empty_like(scaling), torch.empty_like(rotation),
            torch.empty(ng, device=dev), torch.empty_like(feats))
    _lib.check(lib.nlosgr_voxelize_bwd(g, vg, _lib.ptr(cam), opt, _lib.ptr(ws), _lib.ptr(ups[0]), _lib.ptr(ups[1]),
                                       *[_lib.ptr(o) for o in outs], _lib.stream_handle(dev)))
    return outs


class _Raw:
    """The five raw tensors under the reference's attribute names (features [ng, K] split as dc | rest)."""

    def __init__(self, mu, scaling, rotation, opacity, features, deg):
        self._mu, self._scaling, self._rotation, self._opacity = mu, scaling, rotation, opacity
        self._features_dc, self._features_rest = features[:, :1], features[:, 1:]
        self.active_sh_degree = int(deg)


class _VoxelizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, scaling, rotation, opacity, features, grid, cam, preset, cutoff, mod, deg, want_d, want_a):
        raw = _Raw(mu, scaling, rotation, opacity, features, deg)
        dens, alb = voxelize(raw, grid, cam, preset=preset, cutoff=cutoff, scaling_modifier=mod,
                             want_density=want_d, want_albedo=want_a)
        ctx.save_for_backward(mu, scaling, rotation, opacity, features, cam)
        ctx.conf = (grid, preset, cutoff, mod, deg, opacity.shape)
        ctx.set_materialize_grads(False)
        return dens, alb

    @staticmethod
    def backward(ctx, g_dens, g_alb):
        mu, scaling, rotation, opacity, features, cam = ctx.saved_tensors
        grid, preset, cutoff, mod, deg, oshape = ctx.conf
        raw = _Raw(mu, scaling, rotation, opacity, features, deg)
        d_mu, d_s, d_q, d_o, d_f = voxelize_backward(raw, grid, cam, g_dens, g_alb, preset=preset, cutoff=cutoff,
                                                     scaling_modifier=mod)
        return (d_mu, d_s, d_q, d_o.reshape(oshape), d_f) + (None,) * 8


def voxelize_params(mu, scaling, rotation, opacity, features, grid, cam, preset="cuda", cutoff=3.0,
                    scaling_modifier=1.0, sh_degree=0, want_density=True, want_albedo=True):
    """voxelize as a differentiable function of the raw parameter tensors (features [ng, K], as
    model.features_flat lays them out): (density, albedo_density), None where not wanted, the forward exactly
    voxelize's, the backward voxelize_backward.  An output that is not wanted, or that the loss does not
    reach, costs nothing in either direction."""
    return _VoxelizeFn.apply(mu, scaling, rotation, opacity, features, grid, cam, preset, float(cutoff),
                             float(scaling_modifier), int(sh_degree), bool(want_density), bool(want_albedo))


@torch.no_grad()
def project(volume, axis=1):
    """(max, argmax) of volume [nx, ny, nz] along `axis`; argmax is int32, ties go to the lowest index
    (an all-zero column gives (0, 0)); the outputs keep the two remaining axes in their order."""
    lib = _lib.load()
    vol = _gpu_f32(volume, "project")
    if vol.dim() != 3:
        raise ValueError("nlosgr: project needs a [nx, ny, nz] volume")
    if axis not in (0, 1, 2):
        raise ValueError("nlosgr: axis must be 0, 1 or 2")
    shape = [n for a, n in enumerate(vol.shape) if a != axis]
    mx = torch.empty(shape, device=vol.device)
    am = torch.empty(shape, dtype=torch.int32, device=vol.device)
    _lib.check(lib.nlosgr_volume_project(_lib.ptr(vol), vol.shape[0], vol.shape[1], vol.shape[2], int(axis),
                                         _lib.ptr(mx), _lib.ptr(am), _lib.stream_handle(vol.device)))
    return mx, am


@torch.no_grad()
def front_view(volume, grid):
    """(front, depth), each [nx, nz]: the maximum projection along y, the relay wall's normal (walls sit
    at y = 0), and the depth map ys[argmax] — the two images NLOS papers show."""
    mx, am = project(volume, axis=1)
    ys = grid.on(volume.device)[1]
    return mx, ys[am.long()]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nlosgr.voxelize",
                                 description="Voxelize a trained Gaussian checkpoint (density, albedo, front view, depth).")
    ap.add_argument("checkpoint")
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--cutoff", type=float, default=3.0, help="Mahalanobis support radius; <= 0: dense")
    ap.add_argument("--volume-position", type=float, nargs=3, default=(0.0, 0.5, 0.0))
    ap.add_argument("--volume-size", type=float, default=0.5)
    ap.add_argument("--cam", type=float, nargs=3, default=None,
                    help="albedo view point (default: the volume position projected onto the wall y = 0)")
    ap.add_argument("--preset", choices=sorted(_lib.PRESETS), default="torch")
    ap.add_argument("--scaling-modifier", type=float, default=1.0)
    ap.add_argument("--out", default="recon.npz")
    a = ap.parse_args(argv)
    from .checkpoint import load_checkpoint
    if not torch.cuda.is_available():
        raise RuntimeError("nlosgr: voxelize needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    model = load_checkpoint(a.checkpoint, device=dev)
    grid = VoxelGrid(a.volume_position, a.volume_size, a.resolution)
    cam = a.cam if a.cam is not None else (a.volume_position[0], 0.0, a.volume_position[2])
    cam = torch.tensor(cam, dtype=torch.float32, device=dev)
    dens, alb = voxelize(model, grid, cam, preset=a.preset, cutoff=a.cutoff, scaling_modifier=a.scaling_modifier)
    front, depth = front_view(alb, grid)
    np.savez_compressed(a.out, density=dens.cpu().numpy(), albedo=alb.cpu().numpy(), front=front.cpu().numpy(),
                        depth=depth.cpu().numpy(), xs=grid.xs.numpy(), ys=grid.ys.numpy(), zs=grid.zs.numpy(),
                        cam=cam.cpu().numpy())
    print(f"wrote {a.out}: {grid.shape} voxels, {model._mu.shape[0]} Gaussians, cutoff {a.cutoff}")


if __name__ == "__main__":
    main()
