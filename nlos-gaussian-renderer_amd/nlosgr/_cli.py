"""What the command lines that turn a capture into a volume file share (python -m nlosgr.backproject, .phasor,
.forward_project, .fk, .rsd, .lct): the common arguments, opening the capture on the GPU, and the output."""
import argparse

import numpy as np
import torch


def capture_parser(prog, out, description):
    """The parser with the arguments every capture command line has; the module adds its own."""
    ap = argparse.ArgumentParser(prog=prog, description=description)
    ap.add_argument("capture", help="Zaragoza-format .mat file")
    ap.add_argument("--start", type=int, required=True, help="first time bin")
    ap.add_argument("--end", type=int, required=True, help="one past the last time bin")
    ap.add_argument("--out", default=out)
    ap.add_argument("--mesh", default=None, help="also write the isosurface as a PLY file")
    ap.add_argument("--level-frac", type=float, default=0.5, help="isosurface level as a fraction of the maximum")
    return ap


def parse(ap, argv):
    a = ap.parse_args(argv)
    if a.end <= a.start:
        ap.error("--end must be greater than --start")
    return a


def open_capture(path, what):
    """The capture's data_kwargs on cuda:0, unshuffled; RuntimeError("nlosgr: `what` needs a GPU ...") without one."""
    from .data import make_data_kwargs
    if not torch.cuda.is_available():
        raise RuntimeError(f"nlosgr: {what} needs a GPU (no CPU fallback)")
    dk, *_ = make_data_kwargs(path, torch.device("cuda:0"), shuffle=False)
    return dk


def write_volume(a, dk, out, summary, **extra):
    """Write a *_capture result `out` to a.out under the key names of python -m nlosgr.voxelize (density / albedo both
    hold the volume; cam as its default) plus the module's `extra` arrays, print the line that ends in `summary`, and
    write the isosurface to a.mesh when that is given."""
    grid, vol = out["grid"], out["volume"]
    vp = dk["volume_position"].cpu().numpy().astype(np.float32)
    np.savez_compressed(a.out, density=vol.cpu().numpy(), albedo=vol.cpu().numpy(), front=out["front"].cpu().numpy(),
                        depth=out["depth"].cpu().numpy(), xs=grid.xs.numpy(), ys=grid.ys.numpy(), zs=grid.zs.numpy(),
                        cam=np.array([vp[0], 0.0, vp[2]], dtype=np.float32), **extra)
    print(f"wrote {a.out}: {grid.shape} voxels, {dk['camera_grid_positions'].shape[1]} wall points, bins "
          f"[{a.start}, {a.end}), {summary}")
    if a.mesh:
        from .mesh import isosurface, write_ply
        level = a.level_frac * float(vol.max())
        mesh = isosurface(vol, grid, level)
        write_ply(a.mesh, mesh)
        print(f"wrote {a.mesh}: level {level:.6g}, {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} triangles")
