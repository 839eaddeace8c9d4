"""Back-projection timing: nlosgr_backproject (HIP) of a 256 x 256 wall with C3's window (1024 bins of
c deltaT = 1.28 / 1024 from bin 128) onto 128^3 and 64^3 voxels, against what a user could do without it on the
same GPU: the torch composition in chunks of wall points (cdist, floor, gather, sum; written below), and, for
orientation, nlosgr_carve_votes on the same voxel and wall counts (the same distance loop without the gather).
There is no earlier version to compare with.  Warm-up, timed repeats, device-event timing (as
scripts/bench_voxelize.py); writes one JSON file.

    python scripts/bench_backproject.py [--out profiles/backproject_c3.json] [--repeats 5] [--power 0]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nlos-gaussian-renderer_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from nlosgr.backproject import backproject, fp32_window  # noqa: E402
from nlosgr.geometry import relay_wall_grid  # noqa: E402
from nlosgr.init import carve_votes  # noqa: E402
from nlosgr.voxelize import VoxelGrid  # noqa: E402

DEV = torch.device("cuda:0")
POS, SIZE = (0.0, 0.5, 0.0), 0.5
WALL, NR = 256, 1024
DR = 1.28 / NR
R0 = (NR // 8) * DR


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


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "repeats": len(s)}


@torch.no_grad()
def torch_route(rows, walls, grid, r0, dr, power, chunk):
    """The same sum in plain torch: wall points in chunks of `chunk`, each chunk a dense [chunk, Nvox]
    cdist / floor / gather / weighted sum."""
    x = grid.coords().reshape(-1, 3).to(DEV)
    r0, inv_dr = fp32_window(r0, dr)
    nr = rows.shape[1]
    out = torch.zeros(x.shape[0], device=DEV)
    for i in range(0, walls.shape[0], chunk):
        d = torch.cdist(walls[i:i + chunk], x)                                   # [chunk, Nv]
        u = (d - r0) * inv_dr
        k = torch.floor(u)
        f = u - k
        ki = k.long()
        r = rows[i:i + chunk]
        h0 = r.gather(1, ki.clamp(0, nr - 1)) * ((ki >= 0) & (ki < nr))
        h1 = r.gather(1, (ki + 1).clamp(0, nr - 1)) * ((ki >= -1) & (ki < nr - 1))
        s = (1 - f) * h0 + f * h1
        out += (s if power == 0 else d ** power * s).sum(0)
    return out.reshape(grid.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backproject_c3.json"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--power", type=int, default=0)
    ap.add_argument("--torch-chunk", type=int, default=32, help="wall points per torch chunk at 128^3 (256 MiB per [chunk, Nvox] fp32 tensor)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_backproject needs a GPU"
    g = torch.Generator().manual_seed(0)
    walls = relay_wall_grid(WALL, WALL, device=DEV)
    rows = torch.rand(WALL * WALL, NR, generator=g).to(DEV)                      # 268 MB
    radius = torch.full((WALL * WALL,), 0.5, device=DEV)
    res = {"workload": f"{WALL} x {WALL} wall (extent 1 at y = 0), {NR} bins of c deltaT = 1.28 / {NR} from bin {NR // 8} "
                       f"(C3's window), uniform-random rows, seed 0; volume {SIZE} at {POS}; power {a.power}",
           "device": torch.cuda.get_device_name(0), "timing": "device events around each call, median of repeats",
           "evaluation": "one (voxel, wall point) pair: distance, two gathered bins, one term",
           "hip": {}, "torch_chunked": {}, "carve_votes": {}}
    for n in (64, 128):
        grid = VoxelGrid(POS, SIZE, n)
        out = torch.empty(grid.shape, device=DEV)
        evals = n ** 3 * WALL * WALL
        ms = timed(lambda: backproject(rows, walls, grid, R0, DR, power=a.power, out=out), a.warmup, a.repeats)
        e = dict(stats(ms), evaluations=evals)
        e["evaluations_per_s"] = evals / (e["median_ms"] * 1e-3)
        res["hip"][f"{n}^3"] = e
        print("hip", n, e, flush=True)
        coords = grid.coords().reshape(-1, 3).to(DEV).contiguous()
        ms = timed(lambda: carve_votes(coords, walls, radius), a.warmup, a.repeats)
        res["carve_votes"][f"{n}^3"] = stats(ms)
        print("carve", n, res["carve_votes"][f"{n}^3"], flush=True)
        chunk = a.torch_chunk * (128 // n) ** 3
        torch_route(rows[:4 * chunk], walls[:4 * chunk], grid, R0, DR, a.power, chunk)    # warm-up on a part of the wall
        ms = timed(lambda: torch_route(rows, walls, grid, R0, DR, a.power, chunk), 0, 2 if n == 64 else 1)
        t = dict(stats(ms), chunk=chunk)
        ref = torch_route(rows, walls, grid, R0, DR, a.power, chunk)
        t["rel_l2_vs_hip"] = ((out - ref).double().norm() / ref.double().norm()).item()
        t["speedup_hip"] = t["median_ms"] / e["median_ms"]
        res["torch_chunked"][f"{n}^3"] = t
        print("torch", n, t, flush=True)
        del coords, ref
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": "backproject 128^3 x 256^2 x 1024: torch chunked / HIP", "value":
                      res["torch_chunked"]["128^3"]["speedup_hip"]}))


if __name__ == "__main__":
    main()
