"""Voxel-grid oracle shared by test_voxelize_cpu.py and test_gpu_voxelize.py (plain module, no tests).

The two sums nlosgr.voxelize implements, formed from oracle.torch_ref.gaussian_pdf and
oracle.torch_ref.albedo (the restatements of gaussian_model.py:253-294 and :350-355):

    density = sum_g sigma_g pdf_g,   albedo_density = sum_g sigma_g rho_g(cam) pdf_g

test_voxelize_cpu.py pins this formula against the reference's own output (tests/golden/voxel_g32.npz),
so the GPU tests can use it at shapes the fixture does not hold.
"""
import math

import numpy as np
import torch

from oracle import torch_ref as R

H = 0.0125   # voxel spacing of the parity grid


def params_of(model_or_dict, deg, double=False):
    """oracle Params from a dict of arrays (fixture keys) or a model with the reference's attribute names."""
    if isinstance(model_or_dict, dict):
        d = model_or_dict
        vals = [d[k] for k in ("mu", "scaling", "rotation", "opacity", "features_dc", "features_rest")]
    else:
        m = model_or_dict
        vals = [t.detach().cpu() for t in (m._mu, m._scaling, m._rotation, m._opacity, m._features_dc,
                                           m._features_rest)]
    P = R.Params(*vals, deg, requires_grad=False)
    if double:
        for n in ("_mu", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest"):
            setattr(P, n, getattr(P, n).double())
    return P


def volumes(P, coords, cam, preset="torch", mod=1.0, mc=None, band=1e-4):
    """(density, albedo_density, near) over coords [..., 3] in P's dtype; `near` marks the voxels for which
    some Gaussian's m^2 lies within band * mc^2 of mc^2 (the discontinuity of the support mask)."""
    shape = coords.shape[:-1]
    x = coords.reshape(-1, 3).to(P._mu.dtype)
    cam = torch.as_tensor(cam).to(P._mu.dtype)
    with torch.no_grad():
        pdf = R.gaussian_pdf(x, P, preset, mod, None)                     # [Ng, Na]
        near = torch.zeros(x.shape[0], dtype=torch.bool)
        if mc is not None:
            m2 = -2.0 * torch.log(pdf)
            near = ((m2 - mc * mc).abs() <= band * mc * mc).any(dim=0)
            pdf = R.gaussian_pdf(x, P, preset, mod, mc)
        sig = torch.sigmoid(P._opacity).reshape(-1, 1)
        rho = R.albedo(P, cam, preset).reshape(-1, 1)
        dens = torch.sum(pdf * sig, dim=0)
        alb = torch.sum(pdf * sig * rho, dim=0)
    return dens.reshape(shape), alb.reshape(shape), near.reshape(shape)


def parity_axes():
    """40 x 9 x 33 grid of spacing H: no extent is a brick multiple, x and z span two super-bricks."""
    return ((-0.25, -0.25 + 39 * H, 40), (0.45, 0.45 + 8 * H, 9), (-0.2, -0.2 + 32 * H, 33))


PARITY_SEED = 5
PARITY_CAM = (0.03, 0.0, -0.06)


def parity_gaussians(preset, seed=PARITY_SEED):
    """150 Gaussians (raw parameters, SH degree 3) for the parity grid: 145 random ones whose cuda-preset
    supports span about 2 to 6 voxels at cutoff 3 (std in [H/3, H]), then five hand-placed ones:
    centred outside the grid with the support reaching in; support wholly outside; narrower than the voxel
    spacing; covering the whole grid; straddling the super-brick boundary at x index 32 / z index 32.
    Under the torch preset the same raw values apply (every std >= 1 there: all supports cover the grid)."""
    g = torch.Generator().manual_seed(seed)
    n, K = 145, 16
    lo = torch.tensor([-0.27, 0.43, -0.22])
    hi = torch.tensor([0.26, 0.57, 0.22])
    mu = torch.rand(n, 3, generator=g) * (hi - lo) + lo
    if preset == "cuda":
        std = H / 3 + torch.rand(n, 1, generator=g) * (H - H / 3)
        scaling = torch.log(std) + 0.15 * torch.randn(n, 3, generator=g)
    else:
        scaling = torch.randn(n, 3, generator=g) * 0.7 - 1.0
    rotation = torch.randn(n, 4, generator=g)
    opacity = torch.randn(n, 1, generator=g)
    rho = torch.rand(n, 1, generator=g) * 0.2
    fdc = ((rho - 0.5) / R.C0).reshape(n, 1, 1)
    frest = 0.05 * torch.randn(n, K - 1, 1, generator=g)
    hand_mu = torch.tensor([[-0.27, 0.5, 0.0], [0.4, 0.5, 0.0], [0.0135, 0.5005, 0.012], [0.0, 0.5, 0.0],
                            [0.144, 0.5, 0.19]])
    hand_std = torch.tensor([0.012, 0.01, 0.002, 0.5, 0.01])
    m = hand_mu.shape[0]
    cat = lambda a, b: torch.cat((a, b), dim=0)
    return dict(mu=cat(mu, hand_mu), scaling=cat(scaling, torch.log(hand_std).reshape(m, 1).expand(m, 3)),
                rotation=cat(rotation, torch.tensor([[1.0, 0.0, 0.0, 0.0]]).expand(m, 4)),
                opacity=cat(opacity, torch.zeros(m, 1)),
                features_dc=cat(fdc, torch.full((m, 1, 1), (0.3 - 0.5) / R.C0)),
                features_rest=cat(frest, torch.zeros(m, K - 1, 1)))


def grid_coords(axes):
    tabs = [torch.from_numpy(np.linspace(lo, hi, n).astype(np.float32)) for lo, hi, n in axes]
    return torch.stack(torch.meshgrid(*tabs, indexing="ij"), dim=-1)


if __name__ == "__main__":
    # the excluded share of the parity test, measured with the oracle alone (float64)
    for preset in ("torch", "cuda"):
        P = params_of(parity_gaussians(preset), 3, double=True)
        for mc in (3.0, 5.7):
            d, a, near = volumes(P, grid_coords(parity_axes()), PARITY_CAM, preset, 1.0, mc)
            print(preset, mc, "excluded share %.4f%%" % (100.0 * near.float().mean().item()),
                  "density max %.3f" % d.max().item(), "nonzero %.3f" % (d > 0).float().mean().item())
    assert math.isfinite(d.sum().item())
