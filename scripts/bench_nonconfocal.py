"""Non-confocal voxel operators against the confocal ones, timed in the same process: nlosgr_backproject_nc and
nlosgr_forward_project_nc at the shapes of scripts/bench_backproject.py and scripts/bench_forward_project.py (a
256 x 256 wall, C3's window of 1024 bins of c deltaT = 1.28 / 1024 from bin 128, the 0.5 volume at 64^3 and
128^3), each with

    confocal      the confocal entry point (the kernel of the parent commit, unchanged)
    same          lasers == sensors: the general non-confocal kernel on the confocal geometry
    per_meas      one random laser spot on the wall per measurement: the general kernel
    one_laser     one laser spot for the whole capture: the ONE_LASER kernel

The four are timed alternating (one call of each per round), device events around each Python call, median of
--repeats rounds after --warmup untimed rounds.  Writes one JSON file and prints the ratios to the confocal time.

    python scripts/bench_nonconfocal.py [--out profiles/nonconfocal_c3.json] [--repeats 5] [--powers 0 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

POS, SIZE = (0.0, 0.5, 0.0), 0.5
WALL, NR = 256, 1024
DR = 1.28 / NR
R0 = (NR // 8) * DR
GRIDS = (64, 128)
DMIN = 0.25          # the wall is 0.25 in front of the volume: no pair is left out
VARIANTS = ("confocal", "same", "per_meas", "one_laser")


def alternating(fns, warmup, repeats):
    """{name: [ms]}: `repeats` rounds of one call of each function, device events around each call."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "repeats": len(s)}


def summarise(times):
    res = {k: stats(v) for k, v in times.items()}
    base = res["confocal"]["median_ms"]
    for k in res:
        res[k]["ratio_to_confocal"] = res[k]["median_ms"] / base
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nonconfocal_c3.json"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--powers", type=int, nargs="+", default=[0, 2], help="powers of the back-projection; the forward "
                    "projector is timed at these and at their negatives")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nonconfocal needs a GPU"
    from nlosgr.backproject import backproject
    from nlosgr.forward_project import forward_project
    from nlosgr.geometry import relay_wall_grid
    from nlosgr.voxelize import VoxelGrid
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    walls = relay_wall_grid(WALL, WALL, device=dev)
    nm = walls.shape[0]
    per = torch.zeros(nm, 3)
    per[:, 0] = torch.rand(nm, generator=g) - 0.5
    per[:, 2] = torch.rand(nm, generator=g) - 0.5
    lasers = {"same": walls.clone(), "per_meas": per.to(dev), "one_laser": torch.tensor([[-0.45, 0.0, 0.45]], device=dev)}
    rows = torch.rand(nm, NR, generator=g).to(dev)                                # 268 MB
    rows_out = torch.empty(nm, NR, device=dev)
    res = {"workload": f"{WALL} x {WALL} wall (extent 1 at y = 0), {NR} bins of c deltaT = 1.28 / {NR} from bin {NR // 8} "
                       f"(C3's window); volume {SIZE} at {POS}; uniform-random rows, standard-normal dense voxels",
           "device": torch.cuda.get_device_name(0),
           "timing": "the four variants alternating, device events around each call, median of the rounds",
           "backproject": {}, "forward_project": {}}
    for n in GRIDS:
        grid = VoxelGrid(POS, SIZE, n)
        vol = torch.randn(n, n, n, generator=torch.Generator().manual_seed(n)).to(dev)
        vout = torch.empty(grid.shape, device=dev)
        for p in a.powers:
            fns = {"confocal": lambda: backproject(rows, walls, grid, R0, DR, power=p, out=vout)}
            for k, l in lasers.items():
                fns[k] = lambda l=l: backproject(rows, walls, grid, R0, DR, power=p, out=vout, lasers=l)
            e = summarise(alternating(fns, a.warmup, a.repeats))
            res["backproject"][f"{n}^3 power {p}"] = e
            print("backproject", n, p, {k: (round(v["median_ms"], 2), round(v["ratio_to_confocal"], 3)) for k, v in e.items()},
                  flush=True)
        for p in sorted(set(a.powers) | {-q for q in a.powers}):
            fns = {"confocal": lambda: forward_project(vol, walls, grid, R0, DR, NR, power=p, out=rows_out)}
            for k, l in lasers.items():
                fns[k] = lambda l=l: forward_project(vol, walls, grid, R0, DR, NR, power=p, out=rows_out, lasers=l, dmin=DMIN)
            e = summarise(alternating(fns, a.warmup, a.repeats))
            res["forward_project"][f"{n}^3 power {p}"] = e
            print("forward_project", n, p, {k: (round(v["median_ms"], 2), round(v["ratio_to_confocal"], 3)) for k, v in e.items()},
                  flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    b = res["backproject"][f"128^3 power {a.powers[0]}"]
    print(json.dumps({"metric": f"backproject 128^3 power {a.powers[0]}: one_laser / confocal, per_meas / confocal",
                      "value": [b["one_laser"]["ratio_to_confocal"], b["per_meas"]["ratio_to_confocal"]]}))


if __name__ == "__main__":
    main()
