"""Float64 gradient oracle of the voxelizer (plain module, no tests), for test_voxelize_bwd_cpu.py,
test_gpu_voxelize_bwd.py and test_gpu_voxel_fit.py.

    L = sum_x G_d(x) density(x) + sum_x G_a(x) albedo_density(x)

with the two volumes formed in float64 from oracle.torch_ref.gaussian_pdf / albedo (the formula of
voxel_oracle.volumes, pinned there against the reference's own output) and differentiated by torch autograd.

Metric, per gradient tensor and per Gaussian g (the construction of tests/volume_oracle.py):

    G+ / G-   the gradient under the positive / the negative part of the upstream, max(+-G_d, 0), max(+-G_a, 0)
    grads     G+ - G-
    s_g       max_c |G+[g, c]| + max_c |G-[g, c]|      what the row is made of, before the two signs cancel
    e_g       max_c |got[g, c] - grads[g, c]|,  checked as e_g <= tol s_g + u (+ floor_g for d_rotation)

u = 2^-126 2^24 nvox: what fp32 cannot hold.  A pair whose p lies below the smallest normal fp32 number, 2^-126, is
flushed or loses its digits; a row sums at most nvox such pairs, and the chain multiplies the sums by factors (the
entries of N = 1 / s~^2, the upstream, |d|) that stay below 2^24 in these tests.  It matters only for rows whose
whole scale is below about 1e-26, such as a Gaussian hundreds of standard deviations outside the grid in dense mode.

floor_g: an isotropic Gaussian's d_rotation is zero analytically, and float64 autograd returns the rounding of
two equal sums instead (about 1e-16 of the row's terms), so there s_g is the reference's own noise and no
meaningful scale.  d_rotation therefore carries floor_g = 1e-12 s_g(d_scaling): the two rows have the same units
(both parameters are dimensionless) and d_scaling's terms c p u_r^2 never cancel under an upstream of one sign.
1e-12 is far below what fp32 resolves (6e-8), so the floor admits nothing but the reference's noise.
"""
import torch

from oracle import torch_ref as R

NAMES = ("mu", "scaling", "rotation", "opacity", "features")
ATTRS = ("_mu", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")
ROT_FLOOR = 1e-12
UNDERFLOW = 2.0 ** -126 * 2.0 ** 24


def params64(p, deg):
    """Float64 oracle Params with requires_grad leaves, from a dict of arrays (voxel_oracle.parity_gaussians keys)
    or a model with the reference's attribute names."""
    if isinstance(p, dict):
        vals = [p[k] for k in ("mu", "scaling", "rotation", "opacity", "features_dc", "features_rest")]
    else:
        vals = [getattr(p, a).detach().cpu() for a in ATTRS]
    P = R.Params(*vals, deg, requires_grad=False)
    for a in ATTRS:
        setattr(P, a, getattr(P, a).detach().double().clone().requires_grad_(True))
    return P


def volumes64(P, coords, cam, preset, mod=1.0, mc=None):
    """(density, albedo_density) over coords [..., 3] in float64, differentiable in P's leaves."""
    shape = coords.shape[:-1]
    x = coords.reshape(-1, 3).double()
    cam = torch.as_tensor(cam).double()
    pdf = R.gaussian_pdf(x, P, preset, mod, mc)
    sig = torch.sigmoid(P._opacity).reshape(-1, 1)
    rho = R.albedo(P, cam, preset).reshape(-1, 1)
    return torch.sum(pdf * sig, dim=0).reshape(shape), torch.sum(pdf * sig * rho, dim=0).reshape(shape)


def support_mask(P, coords, preset, mod=1.0, mc=None):
    """[Ng, nvox] bool: the pairs in the forward's support (all of them when mc is None)."""
    with torch.no_grad():
        x = coords.reshape(-1, 3).double()
        pdf = R.gaussian_pdf(x, P, preset, mod, None)
        if mc is None:
            return torch.ones_like(pdf, dtype=torch.bool)
        return -2.0 * torch.log(pdf) <= mc * mc


def _five(P, gr):
    """autograd's six tensors (ATTRS order, None allowed) -> name -> [Ng, C] in NAMES' layout."""
    z = [g if g is not None else torch.zeros_like(getattr(P, a)) for g, a in zip(gr, ATTRS)]
    ng = z[0].shape[0]
    return {"mu": z[0], "scaling": z[1], "rotation": z[2], "opacity": z[3].reshape(ng, 1),
            "features": torch.cat((z[4].reshape(ng, -1), z[5].reshape(ng, -1)), dim=1)}


def reference(P, coords, cam, preset, g_dens=None, g_alb=None, mod=1.0, mc=None):
    """(grads, scale): name -> [Ng, C] float64 gradients of L and name -> [Ng] s_g, for upstream volumes
    g_dens / g_alb (coords' leading shape; None: that volume does not enter L)."""
    dens, alb = volumes64(P, coords, cam, preset, mod, mc)
    leaves = [getattr(P, a) for a in ATTRS]
    parts = []
    for s in (1.0, -1.0):
        L = 0.0
        if g_dens is not None:
            L = L + (torch.clamp_min(s * g_dens.double().cpu(), 0.0) * dens).sum()
        if g_alb is not None:
            L = L + (torch.clamp_min(s * g_alb.double().cpu(), 0.0) * alb).sum()
        if not isinstance(L, torch.Tensor):
            parts.append(_five(P, [None] * 6))
            continue
        parts.append(_five(P, torch.autograd.grad(L, leaves, retain_graph=(s > 0), allow_unused=True)))
    grads = {n: parts[0][n] - parts[1][n] for n in NAMES}
    scale = {n: parts[0][n].abs().amax(dim=1) + parts[1][n].abs().amax(dim=1) for n in NAMES}
    return grads, scale


def as_named(five):
    """name -> [Ng, C] float64 on the CPU from the tuple voxelize_backward returns (d_mu, d_scaling, d_rotation,
    d_opacity [ng], d_features)."""
    d_mu, d_s, d_q, d_o, d_f = [t.detach().cpu().double() for t in five]
    return {"mu": d_mu, "scaling": d_s, "rotation": d_q, "opacity": d_o.reshape(-1, 1), "features": d_f}


def ratios(got, grads, scale, nvox):
    """name -> [Ng]: (e_g - u - floor_g)^+ / s_g, the smallest tol Gaussian g passes with (0 where e_g <= floor_g; inf
    where s_g = 0 and e_g is above the floor)."""
    out = {}
    for n in NAMES:
        e = (got[n] - grads[n]).abs().amax(dim=1)
        e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
        floor = UNDERFLOW * nvox + (ROT_FLOOR * scale["scaling"] if n == "rotation" else torch.zeros_like(e))
        ex = torch.clamp_min(e - floor, 0.0)
        out[n] = torch.where(ex > 0, ex / scale[n], torch.zeros_like(ex))
    return out
