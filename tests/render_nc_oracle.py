"""float64 reference of the non-confocal Gaussian renderer and its backward (plain module, no tests; shared by
test_render_nc_cpu.py and test_gpu_render_nc.py).  Built on volume_oracle's tables / directions / Params64 and
oracle.torch_ref's gaussian_pdf / albedo; include/nlosgr.h states the quantity:

    hist[p, k] = hscale[p] att[k] sum_ij sin(theta_i) q_pijk sum_g sigma_g rho_g(s_p) pdf_g(x_pijk)
    x = s_p + d omega_ij,   D = tau_k - c/2,   d = tau_k + (c tau_k / 2 - b^2 / 4) / D,   dl = 2 tau_k - d,
    q = tau_k^2 / (dl D),   Delta = l_p - s_p,  b^2 = |Delta|^2,  c = omega . Delta;   q = 0 where tau_k <= b/2

The fp32 tables and the fp32 laser spots are promoted, so input rounding is shared with the kernel.  With
lasers == sensors d = tau and q = 1 exactly, and hist_nc is volume_oracle.wall_hist's no-occlusion sum.
reference() returns volume_oracle.Reference: the gradient of sum(hist gout) with the per-Gaussian scale s_g (the
positive / negative upstream split) and bracket b_g (dense - culled), exactly as volume_oracle.reference forms them.
"""
import torch

import volume_oracle as VO
from oracle import torch_ref as R


def lasers64(lasers, nmeas):
    """[nmeas, 3] float64 on the CPU from [nmeas, 3] or [1, 3]."""
    l = lasers.detach().cpu().double().reshape(-1, 3)
    return l.expand(nmeas, 3) if l.shape[0] == 1 else l


def points_nc(tab, p, laser):
    """(x [nr, R, 3], sin(theta) [R], q [nr, R]) of measurement p: the sample of every (bin, ray) and its weight; bins
    with tau <= b/2 get q = 0 (their x is the confocal point, which nothing reads)."""
    d, w = VO.directions(tab, p)
    s = tab["wall"][p]
    delta = laser - s
    b2 = (delta * delta).sum()
    c = (d * delta[None, :]).sum(dim=1)[None, :]                      # [1, R]
    tau = tab["r"][:, None]                                           # [nr, 1]
    valid = (tau > 0.5 * torch.sqrt(b2)).expand(tau.shape[0], c.shape[1])
    D = torch.where(valid, tau - 0.5 * c, torch.ones_like(c))
    dist = torch.where(valid, tau + (0.5 * c * tau - 0.25 * b2) / D, tau.expand_as(D))
    dl = 2.0 * tau - dist
    q = torch.where(valid, tau * tau / (dl * D), torch.zeros_like(D))
    return s[None, None, :] + dist[:, :, None] * d[None, :, :], w, q


def hist_nc(P, tab, p, laser, preset, cutoff, culled=None):
    """hist[p, :] (float64, differentiable in P's leaves)."""
    x, w, q = points_nc(tab, p, laser)
    nr, nray = x.shape[0], x.shape[1]
    ng = P._mu.shape[0]
    pdf = R.gaussian_pdf(x.reshape(-1, 3), P, preset, 1.0, VO._mc(cutoff)).view(ng, nr, nray)
    if culled is not None:
        culled.append(int((pdf == 0).sum()))
    sig = torch.sigmoid(P._opacity).reshape(ng, 1, 1)
    rho = R.albedo(P, tab["wall"][p], preset).reshape(ng, 1, 1)
    return tab["hscale"][p] * tab["att"] * (sig * rho * pdf * (w[None, :] * q)[None]).sum(dim=(0, 2))


def forward(P, geo, lasers, preset, cutoff):
    """hist [nmeas, nr] (float64, no graph)."""
    tab = VO.tables(geo)
    n = tab["wall"].shape[0]
    L = lasers64(lasers, n)
    P = VO.Params64(P)
    with torch.no_grad():
        rows = [hist_nc(P, tab, p, L[p], preset, cutoff) for p in range(n)]
    return torch.stack(rows) if rows else torch.zeros(0, tab["r"].shape[0], dtype=torch.float64)


def _split_grads(P, tab, L, preset, cutoff, gout, culled=None):
    hist, G = [], {n: [] for n in VO.NAMES}
    for p in range(tab["wall"].shape[0]):
        h = hist_nc(P, tab, p, L[p], preset, cutoff, culled if VO._mc(cutoff) is not None else None)
        hist.append(h.detach())
        rows = []
        for s in (1.0, -1.0):
            up = torch.clamp_min(s * gout[p], 0.0)
            rows.append(torch.autograd.grad(h, P.leaves(), grad_outputs=up, retain_graph=(s > 0), allow_unused=True))
        for i, n in enumerate(VO.NAMES):
            z = torch.zeros_like(P.leaves()[i])
            G[n].append(torch.stack([(r[i] if r[i] is not None else z).reshape(z.shape[0], -1) for r in rows]))
    return torch.stack(hist), {n: torch.stack(v) for n, v in G.items()}


def reference(P, geo, lasers, preset, cutoff, gout):
    """volume_oracle.Reference of the non-confocal render under the upstream gout [nmeas, nr]."""
    tab = VO.tables(geo)
    L = lasers64(lasers, tab["wall"].shape[0])
    P = VO.Params64(P)
    gout = gout.detach().cpu().double()
    culled = []
    hist, G = _split_grads(P, tab, L, preset, cutoff, gout, culled)
    grads = {n: (g[:, 0] - g[:, 1]).sum(0) for n, g in G.items()}
    scale = {n: VO._rowmax(g).sum(dim=(0, 1)) for n, g in G.items()}
    if VO._mc(cutoff) is None or sum(culled) == 0:
        bracket = {n: torch.zeros_like(scale[n]) for n in VO.NAMES}
        hb = torch.zeros(hist.shape[0], dtype=hist.dtype)
    else:
        dh, DG = _split_grads(P, tab, L, preset, None, gout)
        bracket = {n: VO._rowmax(DG[n] - G[n]).sum(dim=(0, 1)) for n in VO.NAMES}
        hb = (dh - hist).abs().amax(dim=1)
    return VO.Reference(hist, hb, grads, scale, bracket)
