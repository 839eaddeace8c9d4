"""Surface-output timing: nlosgr.mesh (HIP marching tetrahedra) on the density of the C3 synthetic model (100k
Gaussians, cuda preset, SH degree 3) voxelized at 256^3, cutoff 3, at the mean level (the reference's
threshold, nlos_helpers.py:51).  nlosgr_mesh_count and nlosgr_mesh_emit are timed separately (direct C-ABI
calls, outputs allocated once) and together (nlosgr.mesh.isosurface: both calls, the host read of the counts
between them and the output allocation).  Warm-up, device-event timing, median of repeats (as bench.py);
writes one JSON file.

Bytes are the least each phase must move, computed from the shapes (n grid points, nv vertices, nt triangles):
    count   volume read 4n; workspace written 12n (info, vertex offsets, triangle offsets) + block sums;
            workspace read back 4n (info, by the add-back launch) + block sums
    emit    workspace read 8 (nv + nt) (the info word and offset each element starts from); volume read 16 nv
            (both ends' field and value); outputs written 28 nv (position, normal, value) + 12 nt
Neighbour re-reads (the 8 corners of a cell, the 12 gradient taps of an edge) and the bisection probes of the
emit kernels are left to L1 / L2 and are not counted, so GB/s here is a lower bound on the traffic and "share
of HBM peak" is what a perfect streaming implementation would reach in the same time.

    python scripts/bench_mesh.py [--out profiles/mesh_c3.json] [--ng 100000] [--resolution 256] [--repeats 9]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nlosgr  # noqa: E402
from nlosgr import _lib  # noqa: E402
from nlosgr.mesh import isosurface  # noqa: E402
from nlosgr.voxelize import VoxelGrid, voxelize  # noqa: E402

DEV = torch.device("cuda:0")
CAM = (0.0, 0.0, 0.0)
POS, SIZE = (0.0, 0.5, 0.0), 0.5
HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0   # MI355X: 8 TB/s spec, about 6.3 TB/s achievable
SCAN_TILE = 1024                                      # grid points per scan block (kTile, nlosgr_mesh.hip)


def timed(fn, warmup, repeats):
    """Per-call milliseconds (device events around each call), after `warmup` untimed calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def stats(ms, nbytes=None):
    s = sorted(ms)
    out = {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "repeats": len(s)}
    if nbytes is not None:
        gbs = nbytes / (out["median_ms"] * 1e-3) / 1e9
        out.update(min_bytes=int(nbytes), gb_per_s=gbs, share_of_hbm_peak=gbs / HBM_PEAK_GBS,
                   share_of_hbm_achievable=gbs / HBM_ACHIEVABLE_GBS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_c3.json"))
    ap.add_argument("--ng", type=int, default=100000)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh needs a GPU"
    lib = _lib.load()
    model = nlosgr.GaussianParams.synthetic(a.ng, 3, preset="cuda", device=DEV, seed=0)
    cam = torch.tensor(CAM, device=DEV)
    grid = VoxelGrid(POS, SIZE, a.resolution)
    dens, alb = voxelize(model, grid, cam, preset="cuda", cutoff=3.0)
    level = dens.mean().item()
    nx, ny, nz = grid.shape
    n = nx * ny * nz
    xs, ys, zs = grid.on(DEV)
    vg = _lib.VoxelGrid(nx, ny, nz, _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(zs))
    ws_bytes = lib.nlosgr_mesh_workspace_bytes(vg)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    counts = torch.empty(2, dtype=torch.int64, device=DEV)
    stream = _lib.stream_handle(DEV)

    def count():
        _lib.check(lib.nlosgr_mesh_count(_lib.ptr(dens), vg, level, _lib.ptr(ws), _lib.ptr(counts), stream))

    count()
    nv, nt = (int(c) for c in counts.cpu())
    verts, normals = torch.empty(nv, 3, device=DEV), torch.empty(nv, 3, device=DEV)
    vals, faces = torch.empty(nv, device=DEV), torch.empty(nt, 3, dtype=torch.int32, device=DEV)

    def emit():
        _lib.check(lib.nlosgr_mesh_emit(_lib.ptr(dens), _lib.ptr(alb), vg, level, _lib.ptr(ws), nv, nt, _lib.ptr(verts),
                                        _lib.ptr(normals), _lib.ptr(vals), _lib.ptr(faces), stream))

    nblocks = (n + SCAN_TILE - 1) // SCAN_TILE
    count_bytes = {"volume_read": 4 * n, "workspace_written": 12 * n + 4 * nblocks + 16 * nblocks,
                   "workspace_read": 4 * n + 2 * 4 * nblocks + 16 * nblocks}
    emit_bytes = {"workspace_read": 8 * (nv + nt), "volume_read": 16 * nv, "outputs_written": 28 * nv + 12 * nt}
    res = {"workload": f"C3 synthetic model: {a.ng} Gaussians, cuda preset, SH degree 3, seed 0; volume {SIZE} at {POS}; "
                       f"density at {a.resolution}^3, cutoff 3, mean level",
           "device": torch.cuda.get_device_name(0), "timing": "device events around each call, median of repeats",
           "level": level, "density_max": dens.max().item(), "grid_points": n, "vertices": nv, "triangles": nt,
           "workspace_bytes": int(ws_bytes), "hbm_peak_gb_per_s": HBM_PEAK_GBS,
           "hbm_achievable_gb_per_s": HBM_ACHIEVABLE_GBS, "bytes": {"count": count_bytes, "emit": emit_bytes}}
    res["count"] = stats(timed(count, a.warmup, a.repeats), sum(count_bytes.values()))
    print("count", res["count"], flush=True)
    res["emit"] = stats(timed(emit, a.warmup, a.repeats), sum(emit_bytes.values()))
    print("emit", res["emit"], flush=True)
    both = sum(count_bytes.values()) + sum(emit_bytes.values())
    res["count_then_emit"] = stats(timed(lambda: (count(), emit()), a.warmup, a.repeats), both)
    print("count+emit", res["count_then_emit"], flush=True)
    res["isosurface"] = dict(stats(timed(lambda: isosurface(dens, grid, level, values=alb), a.warmup, a.repeats)),
                             note="both calls, the host read of the counts between them, output allocation")
    print("isosurface", res["isosurface"], flush=True)
    m = isosurface(dens, grid, level, values=alb)
    res["bitwise_equal_to_direct_calls"] = bool(torch.equal(m.vertices, verts) and torch.equal(m.normals, normals) and
                                                torch.equal(m.values, vals) and torch.equal(m.faces, faces))
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": f"isosurface {a.resolution}^3 count+emit median ms", "value": res["count_then_emit"]["median_ms"],
                      "vertices": nv, "triangles": nt}))


if __name__ == "__main__":
    main()
