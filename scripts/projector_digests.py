"""One SHA-256 per case of the raw output bytes of the voxel projectors (backproject, forward_project,
phasor_backproject: confocal, a laser per measurement, one laser), from seeded inputs, with the library that
NLOSGR_LIB names (default: the in-tree build).  A refactor of the kernels must leave every digest as it was:

    NLOSGR_LIB=$PWD/ab/libnlosgr_parent.so python scripts/projector_digests.py > before.txt
    python scripts/projector_digests.py > after.txt && cmp before.txt after.txt

(one process per library).  Cases: grids (1,1,1) and (9,5,13) x 1, 3, 257 measurements x 1, 2, 40 bins, every
power of every operator (a negative power where the window allows it: r0 * inv_dr >= 2 confocal, dmin = 0.05
otherwise), the three laser modes, accumulate on and off, forced nsplit 1, 2, 7 beside the library's choice; one
NaN bin, one NaN voxel and an all-zero volume; each operator once at the 64^3 benchmark shape.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
import torch  # noqa: E402

from nlosgr.backproject import backproject, fp32_window  # noqa: E402
from nlosgr.forward_project import forward_project  # noqa: E402
from nlosgr.geometry import relay_wall_grid  # noqa: E402
from nlosgr.phasor import phasor_backproject  # noqa: E402
from nlosgr.voxelize import VoxelGrid  # noqa: E402

DEV = "cuda:0"
R0, FAR, DMIN = 0.3, 0.9, 0.05
COUNT = 0


def emit(name, *tensors):
    global COUNT
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    print(name, h.hexdigest(), flush=True)
    COUNT += 1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def problem(shape, nm, nr):
    g = np.random.default_rng(1000 * nm + nr + sum(shape))
    tabs = [np.linspace(-0.3, 0.3, shape[0]), np.linspace(0.0, 0.6, shape[1]), np.linspace(-0.3, 0.3, shape[2])]
    pts = np.zeros((2, nm, 3), dtype=np.float32)
    pts[:, :, 0], pts[:, :, 2] = g.random((2, nm)) - 0.5, g.random((2, nm)) - 0.5
    return dict(grid=VoxelGrid(tables=[torch.from_numpy(t.astype(np.float32)) for t in tabs]), nr=nr, dr=(FAR - R0) / nr,
                sensors=dev(pts[0]), lasers={"confocal": None, "per_meas": dev(pts[1]), "one_laser": dev(pts[1][:1])},
                rows=dev(g.standard_normal((nm, nr)).astype(np.float32)),
                rows_c=dev(g.standard_normal((nm, nr, 2)).astype(np.float32)),
                vol=dev(g.standard_normal(shape).astype(np.float32)),
                old=dev(g.standard_normal((2,) + shape).astype(np.float32)),
                old_rows=dev(g.standard_normal((nm, nr)).astype(np.float32)))


def gather(tag, c, powers=range(5), rows=None, rows_c=None):
    rows, rows_c = c["rows"] if rows is None else rows, c["rows_c"] if rows_c is None else rows_c
    for mode, las in c["lasers"].items():
        for p in powers:
            for acc in (False, True):
                out = c["old"][0].clone() if acc else None
                emit(f"bp {tag} {mode} p{p} acc{int(acc)}",
                     backproject(rows, c["sensors"], c["grid"], R0, c["dr"], power=p, lasers=las, out=out, accumulate=acc))
                planes = c["old"].clone() if acc else None
                emit(f"ph {tag} {mode} p{p} acc{int(acc)}",
                     *phasor_backproject(rows_c, c["sensors"], c["grid"], R0, c["dr"], power=p, lasers=las, planes=planes,
                                         accumulate=acc))


def scatter(tag, c, powers=range(-4, 5), vol=None, nsplits=(0, 1, 2, 7)):
    vol = c["vol"] if vol is None else vol
    r0, inv_dr = fp32_window(R0, c["dr"])
    for mode, las in c["lasers"].items():
        for p in powers:
            if p < 0 and las is None and not r0 * inv_dr >= 2:
                continue                      # (the library refuses it: no bound on the weight)
            kw = {} if las is None else {"lasers": las, "dmin": DMIN}
            for acc in (False, True):
                for ns in nsplits:
                    out = c["old_rows"].clone() if acc else None
                    emit(f"fp {tag} {mode} p{p} acc{int(acc)} ns{ns}",
                         forward_project(vol, c["sensors"], c["grid"], R0, c["dr"], c["nr"], power=p, out=out,
                                         accumulate=acc, nsplit=ns, **kw))


def main():
    assert torch.cuda.is_available(), "projector_digests needs a GPU"
    for shape in ((1, 1, 1), (9, 5, 13)):
        for nm in (1, 3, 257):
            for nr in (1, 2, 40):
                c = problem(shape, nm, nr)
                tag = f"g{'x'.join(map(str, shape))} m{nm} nr{nr}"
                gather(tag, c)
                scatter(tag, c)
    c = problem((9, 5, 13), 257, 40)
    rows, rows_c, vol = c["rows"].clone(), c["rows_c"].clone(), c["vol"].clone()
    rows[5, 20] = rows_c[5, 20, 1] = vol[4, 2, 6] = float("nan")
    gather("nan-bin", c, powers=(0, 3), rows=rows, rows_c=rows_c)
    scatter("nan-voxel", c, powers=(-2, 0, 3), vol=vol, nsplits=(0, 1))
    scatter("zero-volume", c, powers=(-2, 0, 3), vol=torch.zeros_like(vol), nsplits=(0, 1))
    # the benchmarks' shape: a 256 x 256 wall, 1024 bins of 1.28 / 1024 from bin 128, the 0.5 volume at 64^3
    g = torch.Generator().manual_seed(0)
    walls = relay_wall_grid(256, 256, device=DEV)
    nm, nr, dr = walls.shape[0], 1024, 1.28 / 1024
    grid = VoxelGrid((0.0, 0.5, 0.0), 0.5, 64)
    per = torch.zeros(nm, 3)
    per[:, 0], per[:, 2] = torch.rand(nm, generator=g) - 0.5, torch.rand(nm, generator=g) - 0.5
    rows_c = torch.rand(nm, nr, 2, generator=g).to(DEV)
    rows = rows_c[..., 0].contiguous()
    vol = torch.randn(64, 64, 64, generator=g).to(DEV)
    for mode, las in (("confocal", None), ("per_meas", per.to(DEV)), ("one_laser", per[:1].to(DEV))):
        kw = {} if las is None else {"lasers": las, "dmin": DMIN}
        emit(f"bp 64^3 {mode} p2", backproject(rows, walls, grid, 128 * dr, dr, power=2, lasers=las))
        emit(f"ph 64^3 {mode} p2", *phasor_backproject(rows_c, walls, grid, 128 * dr, dr, power=2, lasers=las))
        emit(f"fp 64^3 {mode} p-1", forward_project(vol, walls, grid, 128 * dr, dr, nr, power=-1, **kw))
    print("cases", COUNT)


if __name__ == "__main__":
    main()
