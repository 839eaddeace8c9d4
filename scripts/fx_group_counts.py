"""Groups formed and split by the FX forward at C3 (nlosgr_fx_info words 5 and 6), with the library NLOSGR_LIB
selects:      python scripts/fx_group_counts.py [order: given|train]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'nlos-gaussian-renderer_amd')); sys.path.insert(0, ROOT)
import torch
from nlosgr import GaussianParams, features_flat
from nlosgr.volume import Scene, make_config
from nlosgr.render import fx_info, render_forward, workspace_for
from nlosgr.train import slab_order, wall_centroid
order = sys.argv[1] if len(sys.argv) > 1 else 'train'
dev = torch.device('cuda:0')
scene = Scene(H=128, W=128, T=1024, ns=32)
m = GaussianParams.synthetic(100_000, 3, preset='cuda', device=dev, seed=0)
geo = scene.geometry(dev, 'cuda')
args = (m._mu.detach(), m._scaling.detach(), m._rotation.detach(), m._opacity.detach(), features_flat(m).detach())
if order == 'train':
    perm = slab_order(args[0], None, 8, 1, size=args[1].max(1).values, centroid=wall_centroid(geo.wall))
    args = tuple(t[perm].contiguous() for t in args)
cfg = make_config(m, scene, 'cuda', cutoff=5.7)
ws = workspace_for(*args, geo, cfg)
render_forward(*args, geo, cfg, workspace=ws)
torch.cuda.synchronize()
i = fx_info(*args, geo, cfg, ws)
print(json.dumps({"lib": os.environ.get("NLOSGR_LIB", "in-tree"), "order": order, "E": i[0], "flushes": i[2],
                  "bright_segments": i[3], "groups": i[4], "splits": i[5]}))
