"""Forward-projection timing: nlosgr_forward_project (HIP) of 64^3 and 128^3 voxels onto a 256 x 256 wall with
C3's window (1024 bins of c deltaT = 1.28 / 1024 from bin 128), for a dense standard-normal volume and one with
2 % non-zeros, against (a) what a user could do without it on the same GPU: the torch composition in chunks of
wall points (cdist, floor, scatter_add_; written below; timed on the first --torch-walls wall points and
scaled to the wall, since its time is linear in them), and (b) nlosgr_backproject on the same counts (the
adjoint does the same pair arithmetic with gathers in place of the scatter's LDS adds).  --ab LIB times the HIP
kernel of an alternative in-tree build as well (a child process started before this one touches the GPU), e.g. the
parent commit's library built from a worktree of it:

    python nlos-gaussian-renderer_amd/build.py --out $OLDPWD/ab/libnlosgr_parent.so

Warm-up, timed repeats, device-event timing (as scripts/bench_backproject.py); writes one JSON file.

    python scripts/bench_forward_project.py [--out profiles/forward_project_c3.json] [--repeats 5] [--power 0]
        [--ab ab/libnlosgr_parent.so ...]
"""
import argparse
import json
import os
import subprocess
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
VOLUMES = ("dense", "sparse2pct")


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


def volume(n, kind, dev):
    g = torch.Generator().manual_seed(n)
    v = torch.randn(n, n, n, generator=g)
    if kind == "sparse2pct":
        v = v * (torch.rand(n, n, n, generator=g) < 0.02)
    return v.to(dev)


@torch.no_grad()
def torch_route(vol, walls, grid, r0, dr, nr, power, chunk):
    """The same sum in plain torch: wall points in chunks of `chunk`, each chunk a dense [chunk, Nvox]
    cdist / floor / two scatter_add_ into rows padded by one bin on either side."""
    from nlosgr.backproject import fp32_window
    dev = vol.device
    x = grid.coords().reshape(-1, 3).to(dev)
    v = vol.reshape(1, -1)
    r0, inv_dr = fp32_window(r0, dr)
    out = torch.empty(walls.shape[0], nr, device=dev)
    for i in range(0, walls.shape[0], chunk):
        d = torch.cdist(walls[i:i + chunk], x)                                   # [chunk, Nv]
        u = (d - r0) * inv_dr
        k = torch.floor(u)
        f = u - k
        wv = v if power == 0 else d ** power * v
        ki = (k.long() + 1).clamp_(0, nr + 1)                                    # padded bin of k; k + 1 follows
        rows = torch.zeros(d.shape[0], nr + 3, device=dev)
        rows.scatter_add_(1, ki, (1 - f) * wv)
        rows.scatter_add_(1, ki + 1, f * wv)
        out[i:i + chunk] = rows[:, 1:nr + 1]
    return out


def hip_times(power, warmup, repeats):
    """{grid: {volume: stats}} of forward_project, plus nlosgr_backproject per grid, with the loaded library."""
    from nlosgr.backproject import backproject
    from nlosgr.forward_project import forward_project
    from nlosgr.geometry import relay_wall_grid
    from nlosgr.voxelize import VoxelGrid
    dev = torch.device("cuda:0")
    walls = relay_wall_grid(WALL, WALL, device=dev)
    out = torch.empty(WALL * WALL, NR, device=dev)
    res = {"hip": {}, "backproject": {}}
    for n in GRIDS:
        grid = VoxelGrid(POS, SIZE, n)
        pairs = n ** 3 * WALL * WALL
        res["hip"][f"{n}^3"] = {}
        for kind in VOLUMES:
            vol = volume(n, kind, dev)
            ms = timed(lambda: forward_project(vol, walls, grid, R0, DR, NR, power=power, out=out), warmup, repeats)
            e = dict(stats(ms), pairs=pairs, nonzero=int((vol != 0).sum()))
            e["pairs_per_s"] = pairs / (e["median_ms"] * 1e-3)
            res["hip"][f"{n}^3"][kind] = e
            print("hip", n, kind, e, flush=True)
        vout = torch.empty(grid.shape, device=dev)
        ms = timed(lambda: backproject(out, walls, grid, R0, DR, power=max(power, 0), out=vout), warmup, repeats)
        res["backproject"][f"{n}^3"] = stats(ms)
        print("backproject", n, res["backproject"][f"{n}^3"], flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_project_c3.json"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--power", type=int, default=0)
    ap.add_argument("--torch-chunk", type=int, default=16, help="wall points per torch chunk at 128^3")
    ap.add_argument("--torch-walls", type=int, default=4096, help="wall points the torch route is timed on")
    ap.add_argument("--ab", action="append", default=[],
                    help="an alternative libnlosgr.so whose HIP kernel is timed as well (may be repeated)")
    ap.add_argument("--hip-only", action="store_true", help="print the HIP timings as one JSON line (the --ab child)")
    a = ap.parse_args()
    ab = {}
    for lib in a.ab:    # each child runs and ends before this process touches the GPU
        env = dict(os.environ, NLOSGR_LIB=os.path.abspath(lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--hip-only", "--power", str(a.power), "--warmup",
                            str(a.warmup), "--repeats", str(a.repeats)], env=env, check=True, capture_output=True, text=True)
        ab[lib] = json.loads(p.stdout.strip().splitlines()[-1])
        print("ab", lib, json.dumps(ab[lib]["hip"]), flush=True)
    assert torch.cuda.is_available(), "bench_forward_project needs a GPU"
    if a.hip_only:
        print(json.dumps(hip_times(a.power, a.warmup, a.repeats)))
        return
    from nlosgr.forward_project import forward_project
    from nlosgr.geometry import relay_wall_grid
    from nlosgr.voxelize import VoxelGrid
    dev = torch.device("cuda:0")
    res = {"workload": f"{WALL} x {WALL} wall (extent 1 at y = 0), {NR} bins of c deltaT = 1.28 / {NR} from bin {NR // 8} "
                       f"(C3's window); volume {SIZE} at {POS}; standard-normal voxels (seed = extent), dense and with "
                       f"2 % non-zeros; power {a.power}",
           "device": torch.cuda.get_device_name(0), "timing": "device events around each call, median of repeats",
           "pair": "one (voxel, wall point) pair: distance, one term, two fixed-point adds"}
    res.update(hip_times(a.power, a.warmup, a.repeats))
    if ab:
        res["ab"] = ab
    res["torch_chunked"] = {}
    walls = relay_wall_grid(WALL, WALL, device=dev)
    for n in GRIDS:
        grid = VoxelGrid(POS, SIZE, n)
        vol = volume(n, "dense", dev)
        chunk = a.torch_chunk * (128 // n) ** 3
        # the torch route's time is linear in the wall points (chunk after chunk): it is timed on the first
        # --torch-walls of them and scaled to the whole wall, which is recorded beside the figure
        nw = min(a.torch_walls, walls.shape[0])
        w = walls[:nw]
        torch_route(vol, w[:2 * chunk], grid, R0, DR, NR, a.power, chunk)        # warm-up on a part of the wall
        keep = []
        ms = timed(lambda: keep.append(torch_route(vol, w, grid, R0, DR, NR, a.power, chunk)), 0, 2 if n == 64 else 1)
        scale = walls.shape[0] / nw
        t = dict(stats([m * scale for m in ms]), chunk=chunk, wall_points_timed=nw, scaled_by=scale)
        ref = keep[-1]
        got = forward_project(vol, w, grid, R0, DR, NR, power=a.power)
        t["rel_l2_vs_hip"] = ((got - ref).double().norm() / ref.double().norm()).item()
        t["speedup_hip"] = t["median_ms"] / res["hip"][f"{n}^3"]["dense"]["median_ms"]
        del keep
        res["torch_chunked"][f"{n}^3"] = t
        print("torch", n, t, flush=True)
        del ref, got
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": "forward_project 128^3 x 256^2 x 1024 dense: torch chunked / HIP", "value":
                      res["torch_chunked"]["128^3"]["speedup_hip"]}))


if __name__ == "__main__":
    main()
