"""Generate the voxel-grid golden fixture by running the REFERENCE's own PyTorch path.

Runs ONLY where the reference checkout is mounted (see make_golden.py, whose import shims and synthetic
parameter recipe it reuses).  It calls

    GaussianModel.estimate_rho_w_no_occlusion(points, cam, c, deltaT, mod, out_separately=True)
                                                              gaussian_model/gaussian_model.py:346-364

on the centres of a 6 x 5 x 7 voxel grid over the hidden volume (meshgrid 'ij' order, linspace tables as
space_carving builds them, gaussian_utils.py:91-93) for 32 Gaussians, at SH degree 3 and 4 and at
scaling modifier 1.0 and 0.7, and writes tests/golden/voxel_g32.npz: inputs (raw parameters, tables,
camera) and the reference's outputs (rho_density, density, rho) only.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_voxel_golden.py
"""
import json
import os

import numpy as np
import torch

from make_golden import HERE, import_reference, synth_params

NG = 32
SHAPE = (6, 5, 7)
DEGS = (3, 4)
MODS = (1.0, 0.7)
VOLUME_POSITION = (0.0, 0.5, 0.0)
VOLUME_SIZE = 0.5
CAM = (0.05, 0.0, -0.1)


def main(out=HERE):
    gu, shu, GaussianModel, H, Config = import_reference()
    tabs = [np.linspace(p - VOLUME_SIZE / 2, p + VOLUME_SIZE / 2, n).astype(np.float32)
            for p, n in zip(VOLUME_POSITION, SHAPE)]
    pts = torch.from_numpy(np.stack(np.meshgrid(*tabs, indexing="ij"), -1).reshape(-1, 3))
    cam = torch.tensor(CAM, dtype=torch.float32)
    c, deltaT = 1.0, 0.01
    rec = dict(xs=tabs[0], ys=tabs[1], zs=tabs[2], cam=cam.numpy())
    for deg in DEGS:
        args = Config().to_namespace()
        args.sh_degree = deg
        p = synth_params(NG, deg, seed=900 + deg)
        model = GaussianModel(args, torch.device("cpu"))
        model._mu = p["mu"].clone()
        model._scaling = p["scaling"].clone()
        model._rotation = p["rotation"].clone()
        model._opacity = p["opacity"].clone()
        model._features_dc = p["features_dc"].clone()
        model._features_rest = p["features_rest"].clone()
        model.max_sh_degree = deg
        model.active_sh_degree = deg
        for k, v in p.items():
            rec[f"d{deg}_{k}"] = v.numpy()
        for mod in MODS:
            with torch.no_grad():
                rho_density, density, rho = model.estimate_rho_w_no_occlusion(pts, cam, c, deltaT, mod,
                                                                             out_separately=True)
            tag = f"d{deg}_m{str(mod).replace('.', 'p')}"
            rec[f"{tag}_rho_density"] = rho_density.numpy().reshape(SHAPE)
            rec[f"{tag}_density"] = density.numpy().reshape(SHAPE)
            rec[f"{tag}_rho"] = rho.numpy()
            print(tag, "density max", float(density.max()), "rho_density max", float(rho_density.max()))
    rec["meta"] = np.array(json.dumps(dict(ng=NG, shape=SHAPE, degs=DEGS, mods=MODS, volume_size=VOLUME_SIZE,
                                           volume_position=VOLUME_POSITION, torch_version=torch.__version__)))
    np.savez_compressed(os.path.join(out, "voxel_g32.npz"), **rec)


if __name__ == "__main__":
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    main()
