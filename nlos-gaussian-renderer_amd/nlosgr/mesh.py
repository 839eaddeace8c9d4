"""Surface output: the isosurface of a voxelized field as a triangle mesh, written as PLY.

The reference's evaluation() gets a surface from gaussian2volume(mode='mesh') (nlos_helpers.py:50-69): it
thresholds the density at its mean (:51) and runs open3d's Poisson reconstruction.  The density here is
already a regular-grid scalar field on the device (nlosgr.voxelize), so the surface the reference wants,
{x : density(x) = mean density}, is extracted directly as an isosurface: marching tetrahedra on the Kuhn
decomposition (nlosgr_mesh_count / nlosgr_mesh_emit, include/nlosgr.h "Surface output"), watertight by
construction, no atomics, a fixed vertex and triangle order, bitwise repeatable.  No CPU fallback.

    python -m nlosgr.mesh CKPT --resolution 256 --cutoff 3 --volume-position x y z --volume-size s \
        [--level L | --level-frac F] [--field density|albedo] --out mesh.ply
"""
import argparse
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .voxelize import VoxelGrid, _gpu_f32, voxelize

MAX_ELEMENTS = 2 ** 31 - 1   # int32 indices

Mesh = namedtuple("Mesh", ["vertices", "normals", "values", "faces"])
Mesh.__doc__ = """vertices [nv,3] fp32, normals [nv,3] fp32 (unit, from high field values to low; zero where the
gradient vanishes), values [nv] fp32 or None, faces [nt,3] int32 (counter-clockwise seen from the low side)."""


@torch.no_grad()
def isosurface(volume, grid, level, values=None):
    """Mesh of {volume = level}: volume [nx,ny,nz] fp32 on the GPU over `grid` (a VoxelGrid, tables read as
    given); `values`, an optional second volume of the same shape, is interpolated to the vertices.
    nlosgr_mesh_count, one .cpu() of the two counts (the only synchronisation: the outputs cannot be sized
    without it), nlosgr_mesh_emit, all on the current stream."""
    lib = _lib.load()
    vol = _gpu_f32(volume, "isosurface")
    attr = _gpu_f32(values, "isosurface") if values is not None else None
    if vol.dim() != 3 or tuple(vol.shape) != grid.shape:
        raise ValueError("nlosgr: isosurface needs a [nx, ny, nz] volume of the grid's shape")
    if attr is not None and attr.shape != vol.shape:
        raise ValueError("nlosgr: values must have the volume's shape")
    dev = vol.device
    xs, ys, zs = grid.on(dev)
    nx, ny, nz = grid.shape
    vg = _lib.VoxelGrid(nx, ny, nz, _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(zs))
    nbytes = lib.nlosgr_mesh_workspace_bytes(vg)
    if nbytes == 0:
        _lib.check(1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    stream = _lib.stream_handle(dev)
    _lib.check(lib.nlosgr_mesh_count(_lib.ptr(vol), vg, float(level), _lib.ptr(ws), _lib.ptr(counts), stream))
    nv, nt = (int(c) for c in counts.cpu())
    if nv > MAX_ELEMENTS or nt > MAX_ELEMENTS:
        raise RuntimeError(f"nlosgr: isosurface has {nv} vertices and {nt} triangles; at most {MAX_ELEMENTS} "
                           "of each are supported (int32 indices): lower the resolution or raise the level")
    verts = torch.empty(nv, 3, device=dev)
    normals = torch.empty(nv, 3, device=dev)
    vals = torch.empty(nv, device=dev) if attr is not None else None
    faces = torch.empty(nt, 3, dtype=torch.int32, device=dev)
    if nv > 0:
        _lib.check(lib.nlosgr_mesh_emit(_lib.ptr(vol), _lib.ptr(attr), vg, float(level), _lib.ptr(ws), nv, nt,
                                        _lib.ptr(verts), _lib.ptr(normals), _lib.ptr(vals), _lib.ptr(faces), stream))
    return Mesh(verts, normals, vals, faces)


@torch.no_grad()
def extract_mesh(model, grid, cam, level=None, level_frac=None, field="density", preset="cuda", cutoff=3.0,
                 scaling_modifier=1.0, sh_degree=None):
    """(mesh, level): voxelize `model` on `grid` (arguments as nlosgr.voxelize.voxelize) and extract the
    isosurface of `field` ('density' or 'albedo'); the other field is interpolated to the vertices as
    mesh.values.  level=None: the field's mean, the reference's threshold (nlos_helpers.py:51);
    level_frac=F: F x the field's maximum.  Reading the level is one more host synchronisation."""
    if field not in ("density", "albedo"):
        raise ValueError("nlosgr: field must be 'density' or 'albedo'")
    if level is not None and level_frac is not None:
        raise ValueError("nlosgr: give level or level_frac, not both")
    dens, alb = voxelize(model, grid, cam, preset=preset, cutoff=cutoff, scaling_modifier=scaling_modifier,
                         sh_degree=sh_degree)
    f, other = (dens, alb) if field == "density" else (alb, dens)
    if level_frac is not None:
        level = float(level_frac) * f.max().item()
    elif level is None:
        level = f.mean().item()
    return isosurface(f, grid, float(level), values=other), float(level)


def write_ply(path, mesh):
    """Binary little-endian PLY: vertex x y z nx ny nz (float) [+ value (float)], face list uchar int."""
    v = np.asarray(torch.as_tensor(mesh.vertices).cpu().numpy(), dtype="<f4").reshape(-1, 3)
    n = np.asarray(torch.as_tensor(mesh.normals).cpu().numpy(), dtype="<f4").reshape(-1, 3)
    f = np.asarray(torch.as_tensor(mesh.faces).cpu().numpy(), dtype="<i4").reshape(-1, 3)
    cols = [v, n]
    props = ["x", "y", "z", "nx", "ny", "nz"]
    if mesh.values is not None:
        cols.append(np.asarray(torch.as_tensor(mesh.values).cpu().numpy(), dtype="<f4").reshape(-1, 1))
        props.append("value")
    if n.shape != v.shape or any(c.shape[0] != v.shape[0] for c in cols):
        raise ValueError("nlosgr: write_ply needs one normal (and value) per vertex")
    header = ["ply", "format binary_little_endian 1.0", "comment nlosgr isosurface", f"element vertex {v.shape[0]}"]
    header += [f"property float {p}" for p in props]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    face_rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face_rec["n"] = 3
    face_rec["i"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(np.ascontiguousarray(np.concatenate(cols, axis=1)).tobytes())
        fh.write(face_rec.tobytes())


def read_ply(path):
    """Mesh of numpy arrays from a PLY written by write_ply (binary little-endian, float vertex properties,
    triangles only)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("nlosgr: read_ply reads binary little-endian PLY only")
    counts, props, cur = {}, {"vertex": [], "face": []}, None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            cur = w[1]
            counts[cur] = int(w[2])
            props.setdefault(cur, [])
        elif w[:1] == ["property"]:
            props[cur].append(w[1:])
    vp = props["vertex"]
    if any(p[0] != "float" for p in vp) or [p[1] for p in vp[:6]] != ["x", "y", "z", "nx", "ny", "nz"]:
        raise ValueError("nlosgr: read_ply needs float vertex properties x y z nx ny nz [value]")
    if props["face"] != [["list", "uchar", "int", "vertex_indices"]]:
        raise ValueError("nlosgr: read_ply needs faces as 'list uchar int vertex_indices'")
    nv, nf, k = counts["vertex"], counts["face"], len(vp)
    tab = np.frombuffer(data, dtype="<f4", count=nv * k, offset=end).reshape(nv, k)
    rec = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=end + 4 * nv * k)
    if nf and (rec["n"] != 3).any():
        raise ValueError("nlosgr: read_ply reads triangles only")
    vals = tab[:, 6].copy() if k > 6 and vp[6][1] == "value" else None
    return Mesh(tab[:, 0:3].copy(), tab[:, 3:6].copy(), vals, rec["i"].astype(np.int32).reshape(nf, 3))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nlosgr.mesh",
                                 description="Isosurface mesh (PLY) of a trained Gaussian checkpoint's voxelized field.")
    ap.add_argument("checkpoint")
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--cutoff", type=float, default=3.0, help="Mahalanobis support radius; <= 0: dense")
    ap.add_argument("--volume-position", type=float, nargs=3, default=(0.0, 0.5, 0.0))
    ap.add_argument("--volume-size", type=float, default=0.5)
    ap.add_argument("--cam", type=float, nargs=3, default=None,
                    help="albedo view point (default: the volume position projected onto the wall y = 0)")
    lv = ap.add_mutually_exclusive_group()
    lv.add_argument("--level", type=float, default=None, help="iso level (default: the field's mean)")
    lv.add_argument("--level-frac", type=float, default=None, help="iso level as a fraction of the field's maximum")
    ap.add_argument("--field", choices=("density", "albedo"), default="density")
    ap.add_argument("--preset", choices=sorted(_lib.PRESETS), default="torch")
    ap.add_argument("--scaling-modifier", type=float, default=1.0)
    ap.add_argument("--out", default="mesh.ply")
    a = ap.parse_args(argv)
    from .checkpoint import load_checkpoint
    if not torch.cuda.is_available():
        raise RuntimeError("nlosgr: mesh needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    model = load_checkpoint(a.checkpoint, device=dev)
    grid = VoxelGrid(a.volume_position, a.volume_size, a.resolution)
    cam = a.cam if a.cam is not None else (a.volume_position[0], 0.0, a.volume_position[2])
    cam = torch.tensor(cam, dtype=torch.float32, device=dev)
    mesh, level = extract_mesh(model, grid, cam, level=a.level, level_frac=a.level_frac, field=a.field,
                               preset=a.preset, cutoff=a.cutoff, scaling_modifier=a.scaling_modifier)
    write_ply(a.out, mesh)
    print(f"wrote {a.out}: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} triangles, "
          f"{a.field} level {level:.9g}, {grid.shape} voxels")


if __name__ == "__main__":
    main()
