"""Counters of the FX forward drain (debug build -DNLOSGR_FXCOUNT, selected by NLOSGR_LIB), per launch.
Refills: the refills of the drain loop, the queue entries they took, the refills that took fewer than 32 entries
and the refills after the chunk's enumeration had ended, next to the drain rounds (scripts/refill_replay.py
prints the same five numbers from a CPU replay of the loop).  Bank-pair occupancy, per drain round: the active
lanes, the sum over the 4 16-lane groups of the largest number of lanes on one bank pair (the ds_add_u64's
LDS-array cycles; 4 = conflict-free), the distinct bank pairs in the wave and the wave's largest residue count.
Support: the rays taken with bins (a twin counts two) and, with `trim` (FLAG_FX_TRIM, what TrainStep sets), the
pairs dropped because they peak below a quarter unit; scripts/trim_estimate.py predicts both on the CPU.
    python scripts/fx_counts.py [order: given|train] [scene: c3|small] [support: full|trim]
(small: the 1500 Gaussians, 3 x 3 wall points, 256 bins, ns 16 of tests/test_gpu_fx_refill.py)"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'nlos-gaussian-renderer_amd')); sys.path.insert(0, ROOT)
import torch
from nlosgr import GaussianParams, features_flat, _lib
from nlosgr.volume import Scene, make_config
from nlosgr.render import render_forward
from nlosgr.train import slab_order, wall_centroid
order = sys.argv[1] if len(sys.argv) > 1 else 'train'
which = sys.argv[2] if len(sys.argv) > 2 else 'c3'
trim = (sys.argv[3] if len(sys.argv) > 3 else 'full') == 'trim'
dev = torch.device('cuda:0')
if which == 'small':
    scene = Scene(H=3, W=3, T=256, ns=16)
    m = GaussianParams.synthetic(1500, 3, preset='cuda', device=dev, seed=21)
else:
    scene = Scene(H=128, W=128, T=1024, ns=32)
    m = GaussianParams.synthetic(100_000, 3, preset='cuda', device=dev, seed=0)
geo = scene.geometry(dev, 'cuda')
args = (m._mu.detach(), m._scaling.detach(), m._rotation.detach(), m._opacity.detach(), features_flat(m).detach())
if order == 'train':
    perm = slab_order(args[0], None, 8, 1, size=args[1].max(1).values, centroid=wall_centroid(geo.wall))
    args = tuple(t[perm].contiguous() for t in args)
cfg = make_config(m, scene, 'cuda', cutoff=5.7)
if trim:
    from dataclasses import replace
    cfg = replace(cfg, flags=_lib.FLAG_FX_TRIM)
lib = _lib.load()
f = lib.nlosgr_debug_fx_counts
f.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
buf = (ctypes.c_ulonglong * 12)()
torch.cuda.synchronize(); f(buf)
render_forward(*args, geo, cfg)
torch.cuda.synchronize(); f(buf)
c = list(buf)
r = max(c[0], 1)
print(json.dumps({"lib": os.environ.get("NLOSGR_LIB", "in-tree"), "order": order, "scene": which, "support": "trim" if trim else "full",
                  "rounds": c[0], "rays_taken": c[9], "pairs_dropped": c[10],
                  "refills": c[5], "entries_taken": c[6], "refills_under_32": c[7], "refills_in_tail": c[8],
                  "entries_per_refill": c[6] / max(c[5], 1), "refills_per_round": c[5] / r,
                  "active_per_round": c[1] / r, "sum_group_max_per_round": c[2] / r,
                  "distinct_residues_per_round": c[3] / r, "wave_max_residue_count_per_round": c[4] / r}))
