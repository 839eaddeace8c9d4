"""float64 reference of the batched volume render and its backward, and the per-Gaussian metric the backward
is judged by (plain module, no tests; shared by test_volume_oracle_cpu.py and test_gpu_bwd_edges.py).

The reference promotes the fp32 tables the kernels read (nlosgr.geometry.Geometry: wall, sin/cos theta,
sin/cos phi, r, att, hscale), so input rounding is shared with the kernel and only its arithmetic is measured:

    hist[p, k] = hscale[p] att[k] sum_g sum_ij sin(theta_i) val_g(x_pijk)
    x_pijk     = wall_p + r_k (sin(theta_i) cos(phi_j), sin(theta_i) sin(phi_j), cos(theta_i))
    noocl      val = sigma_g rho_g(p) pdf_g
    netf       D = sigma pdf, f = exp(-D c dT) + 1e-7, T = exclusive cumprod of f along k, val = D T rho c dT

pdf and rho are oracle.torch_ref.gaussian_pdf / albedo in double; cutoff None (or <= 0) is the dense sum,
otherwise the support mask is m^2 <= cutoff^2.  Gradients are torch autograd through these sums.

The per-Gaussian metric.  With G[p, s] the gradient under the upstream row max(s gout[p], 0), s = +-1, and all
other rows zero (the backward is linear in the upstream, so the gradient itself is sum_p G[p, +] - G[p, -]):

    scale    s_g = sum_{p, s} max_c |G[p, s][g, c]|           what Gaussian g's row is made of, before cancellation
    bracket  b_g = sum_{p, s} max_c |Gdense[p, s] - G[p, s]|  at cutoff >= 5 the kernel's TAIL drains add the exact
                                                              tail of a segment's last round, so its result lies
                                                              between the culled and the dense reference
    error    e_g = max_c |got[g, c] - ref[g, c]|,   checked as e_g <= tol s_g + b_g for every Gaussian

per gradient tensor (NAMES).  A plain row maximum would not do for s_g: a Gaussian whose net d_opacity nearly
cancels under a random upstream shows the fp32 oracle itself 7e-4 away relative to that maximum.  Gaussians no
sample reaches have s_g = 0 and must come out within b_g.  The forward is judged per row: |got - ref| against
tol times the row's own maximum plus the row's bracket max_k |dense - culled|.
"""
from dataclasses import dataclass

import torch

from oracle import torch_ref as R

NAMES = ("mu", "scaling", "rotation", "opacity", "features_dc", "features_rest")
_LEAVES = ("_mu", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")


class Params64(R.Params):
    """oracle Params promoted to float64 leaves that require grad (from fp32 or fp64 Params)."""

    def __init__(self, src):
        for n in _LEAVES:
            setattr(self, n, getattr(src, n).detach().cpu().double().clone().requires_grad_(True))
        self.active_sh_degree = int(src.active_sh_degree)


def tables(geo):
    """The fp32 tables the kernel reads, promoted to float64 on the CPU."""
    f = lambda t: t.detach().cpu().double()
    return dict(wall=f(geo.wall), st=f(geo.sin_theta), ct=f(geo.cos_theta), sp=f(geo.sin_phi), cp=f(geo.cos_phi),
                r=f(geo.r), att=f(geo.att), hscale=f(geo.hscale))


def directions(tab, p):
    """[nt * np, 3] unit ray directions of wall point p, rays in (i, j) order, and sin(theta) per ray."""
    st, ct, sp, cp = tab["st"][p], tab["ct"][p], tab["sp"][p], tab["cp"][p]
    nt, nph = st.shape[0], sp.shape[0]
    d = torch.stack([st[:, None] * cp[None, :], st[:, None] * sp[None, :], ct[:, None].expand(nt, nph)], dim=-1)
    return d.reshape(-1, 3), st[:, None].expand(nt, nph).reshape(-1)


def _rowmax(t):
    """max_c |t[..., c]| (zeros for a tensor without columns, e.g. features_rest at SH degree 0)."""
    return t.abs().amax(dim=-1) if t.shape[-1] else torch.zeros(t.shape[:-1], dtype=t.dtype)


def _mc(cutoff):
    return float(cutoff) if cutoff is not None and cutoff > 0 else None


def _points(tab, p):
    d, w = directions(tab, p)
    x = tab["wall"][p][None, None, :] + tab["r"][:, None, None] * d[None, :, :]      # [nr, R, 3]
    return x, w


def wall_hist(P, tab, p, preset, mode, c_deltaT, cutoff, culled=None):
    """hist[p, :] (float64, differentiable in P's leaves); the number of samples the mask removed is appended
    to the list `culled`."""
    x, w = _points(tab, p)
    nr, nray = x.shape[0], x.shape[1]
    ng = P._mu.shape[0]
    pdf = R.gaussian_pdf(x.reshape(-1, 3), P, preset, 1.0, _mc(cutoff)).view(ng, nr, nray)
    if culled is not None:   # (a double pdf is never 0 inside a support of a few sigma)
        culled.append(int((pdf == 0).sum()))
    sig = torch.sigmoid(P._opacity).reshape(ng, 1, 1)
    rho = R.albedo(P, tab["wall"][p], preset).reshape(ng, 1, 1)
    if mode == "noocl":
        val = sig * rho * pdf
    elif mode == "netf":
        D = sig * pdf
        f = torch.exp(-D * c_deltaT) + 1e-7
        T = torch.cat([torch.ones_like(f[:, :1]), torch.cumprod(f, dim=1)[:, :-1]], dim=1)
        val = D * T * rho * c_deltaT
    else:
        raise ValueError(mode)
    return tab["hscale"][p] * tab["att"] * (val * w[None, None, :]).sum(dim=(0, 2))


def support_mask(P, geo, preset, cutoff):
    """bool [P, Ng, nr, rays]: the samples with m^2 <= cutoff^2 (all of them when dense)."""
    tab = tables(geo)
    out = []
    with torch.no_grad():
        for p in range(tab["wall"].shape[0]):
            x, _ = _points(tab, p)
            pdf = R.gaussian_pdf(x.reshape(-1, 3), P, preset, 1.0, _mc(cutoff))
            out.append((pdf > 0).view(P._mu.shape[0], x.shape[0], x.shape[1]))
    return torch.stack(out)


def forward(P, geo, preset, mode, c_deltaT, cutoff):
    """hist [P, nr] (float64, no graph)."""
    tab = tables(geo)
    P = Params64(P)
    with torch.no_grad():
        return torch.stack([wall_hist(P, tab, p, preset, mode, c_deltaT, cutoff) for p in range(tab["wall"].shape[0])])


def _split_grads(P, tab, preset, mode, c_deltaT, cutoff, gout, culled=None):
    """hist [P, nr] and, per tensor, G [P, 2, Ng, C]: the gradient under max(+gout[p], 0) / max(-gout[p], 0)."""
    nw = tab["wall"].shape[0]
    hist, G = [], {n: [] for n in NAMES}
    for p in range(nw):
        h = wall_hist(P, tab, p, preset, mode, c_deltaT, cutoff, culled)
        hist.append(h.detach())
        rows = []
        for s in (1.0, -1.0):
            up = torch.clamp_min(s * gout[p], 0.0)
            rows.append(torch.autograd.grad(h, P.leaves(), grad_outputs=up, retain_graph=(s > 0), allow_unused=True))
        for i, n in enumerate(NAMES):
            z = torch.zeros_like(P.leaves()[i])
            G[n].append(torch.stack([(r[i] if r[i] is not None else z).reshape(z.shape[0], -1) for r in rows]))
    return torch.stack(hist), {n: torch.stack(v) for n, v in G.items()}


@dataclass
class Reference:
    hist: torch.Tensor          # [P, nr]
    hist_bracket: torch.Tensor  # [P]   max_k |dense - culled|
    grads: dict                 # name -> [Ng, C]
    scale: dict                 # name -> [Ng]   s_g
    bracket: dict               # name -> [Ng]   b_g


def reference(P, geo, preset, mode, c_deltaT, cutoff, gout):
    """The float64 forward, gradients under the upstream gout [P, nr], and the metric's s_g and b_g."""
    tab = tables(geo)
    P = Params64(P)
    gout = gout.detach().cpu().double()
    culled = []
    hist, G = _split_grads(P, tab, preset, mode, c_deltaT, cutoff, gout, culled)
    grads = {n: (g[:, 0] - g[:, 1]).sum(0) for n, g in G.items()}
    scale = {n: _rowmax(g).sum(dim=(0, 1)) for n, g in G.items()}
    if _mc(cutoff) is None or sum(culled) == 0:   # nothing culled: the dense reference is the same sum
        bracket = {n: torch.zeros_like(scale[n]) for n in NAMES}
        hb = torch.zeros(hist.shape[0], dtype=hist.dtype)
    else:
        dh, DG = _split_grads(P, tab, preset, mode, c_deltaT, None, gout)
        bracket = {n: _rowmax(DG[n] - G[n]).sum(dim=(0, 1)) for n in NAMES}
        hb = (dh - hist).abs().amax(dim=1)
    return Reference(hist, hb, grads, scale, bracket)


def as_named(grads):
    """name -> [Ng, C] float64 from six tensors in NAMES order, or from render_backward's five (d_mu, d_scaling,
    d_rotation, d_opacity, d_features [Ng, K]: column 0 is features_dc, the rest features_rest)."""
    g = [t.detach().cpu().double() for t in grads]
    if len(g) == 5:
        ng = g[0].shape[0]
        f = g[4].reshape(ng, -1)
        g = g[:4] + [f[:, :1], f[:, 1:]]
    ng = g[0].shape[0]
    return {n: t.reshape(ng, -1) for n, t in zip(NAMES, g)}


def gaussian_errors(got, ref):
    """name -> e_g [Ng]."""
    got = got if isinstance(got, dict) else as_named(got)
    return {n: _rowmax(got[n] - ref.grads[n]) for n in NAMES}


def _tol(tol, n):
    """tol: one number, name -> number, or name -> [Ng] (a tolerance per Gaussian)."""
    t = tol[n] if isinstance(tol, dict) else tol
    return t.double() if torch.is_tensor(t) else float(t)


def failures(got, ref, tol):
    """[(name, g, e_g, s_g, b_g)] of every Gaussian with e_g > tol s_g + b_g (tol: see _tol).
    The bracket gets one part in 1e9 of slack (it is a difference of two float64 sums)."""
    out = []
    for n, e in gaussian_errors(got, ref).items():
        s, b = ref.scale[n], ref.bracket[n]
        bad = torch.nonzero(~(e <= _tol(tol, n) * s + b * (1 + 1e-9))).flatten()   # (a NaN fails)
        out += [(n, int(g), float(e[g]), float(s[g]), float(b[g])) for g in bad]
    return out


def relative_errors(got, ref):
    """name -> [Ng]: (e_g - b_g)^+ / s_g, the smallest tol Gaussian g passes with (0 where s_g = 0)."""
    out = {}
    for n, e in gaussian_errors(got, ref).items():
        s, b = ref.scale[n], ref.bracket[n]
        out[n] = torch.where(s > 0, torch.clamp_min(e - b, 0.0) / s.clamp_min(1e-300), torch.zeros_like(s))
    return out


def worst(got, ref):
    """name -> the smallest tol that passes: max over the Gaussians with s_g > 0 of (e_g - b_g)^+ / s_g."""
    return {n: float(v.max()) if v.numel() else 0.0 for n, v in relative_errors(got, ref).items()}


def conditioning(P, geo, preset):
    """What makes a Gaussian hard in fp32, from the scene alone (float64): per Gaussian the largest whitened
    distance of a wall point, |u0| = max_p |S^-1 R (wall_p - mu)| (the kernels evaluate a sample's whitened
    position as u0 + r v, two vectors of that size whose sum is at most the cutoff), and its smallest standard
    deviation in bins, sigma_b = min(s) / dr.  Returns (u0 [Ng], sigma_b [Ng])."""
    P = Params64(P)
    with torch.no_grad():
        tab = tables(geo)
        wall = tab["wall"]
        dr = float(tab["r"][-1] - tab["r"][0]) / max(tab["r"].shape[0] - 1, 1)
        if preset == "torch":
            s = torch.exp(torch.exp(P._scaling))
            rot = R.build_rotation(torch.nn.functional.normalize(P._rotation))
        else:
            s = torch.exp(P._scaling) + 1e-8
            rot = R.quat_to_rotmat_cuda(P._rotation).transpose(1, 2)
        q = wall[None, :, :] - P._mu[:, None, :]                                    # [Ng, P, 3]
        u0 = torch.einsum("gab,gpb->gpa", rot, q) / s[:, None, :]
        return u0.norm(dim=-1).amax(dim=1), s.amin(dim=1) / dr


def unreached_failures(got, ref):
    """[(name, g, e_g, b_g)] of the Gaussians with s_g = 0 that do not come out within b_g."""
    out = []
    for n, e in gaussian_errors(got, ref).items():
        dead = ref.scale[n] == 0
        bad = torch.nonzero(dead & ~(e <= ref.bracket[n] * (1 + 1e-9))).flatten()
        out += [(n, int(g), float(e[g]), float(ref.bracket[n][g])) for g in bad]
    return out


def forward_worst(hist, ref):
    """max over rows of (max_k |hist - ref| - bracket)^+ / the row's maximum; rows the reference leaves empty
    must come out within their bracket (inf otherwise)."""
    h = hist.detach().cpu().double()
    err = torch.clamp_min((h - ref.hist).abs().amax(dim=1) - ref.hist_bracket * (1 + 1e-9), 0.0)
    top = ref.hist.abs().amax(dim=1)
    rel = torch.where(top > 0, err / top.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                         torch.zeros_like(err)))
    return float(rel.max())


# --------------------------------------------------------------------------------------------
# scenes shared by the CPU and the GPU tests
# --------------------------------------------------------------------------------------------
def parity_scene(preset, mode, T, device=None, scale_shift=None, ng=48, ns=6, wall=(2, 3), seed=3, edit=None):
    """The scene of tests/test_gpu_parity.py::_volume_vs_oracle: `ng` synthetic Gaussians of SH degree 3 (cuda
    preset: log-scales + 1.2, or + scale_shift), a 2 x 3 relay wall, ns x ns rays, T bins of 1.28 / T from bin
    T // 8.  edit(model, walls) may change the parameters in place.  Returns (model, geo, consts) with consts =
    dict(walls, box, ns, start, end, c, deltaT, Y) as oracle.torch_ref.render_volume takes them."""
    from nlosgr import GaussianParams
    from nlosgr.geometry import build_geometry, relay_wall_grid, volume_box_point
    c, deltaT = 1.0, 1.28 / T
    start, end = T // 8, T // 8 + T
    model = GaussianParams.synthetic(ng, 3, preset=preset, device=device, seed=seed)
    walls = relay_wall_grid(wall[0], wall[1], device=device)
    with torch.no_grad():
        if preset == "cuda":
            model._scaling.add_(1.2 if scale_shift is None else scale_shift)
        if edit is not None:
            edit(model, walls)
    box = volume_box_point((0.0, 0.5, 0.0), 0.5, device)
    geo = build_geometry(walls, box, ns, start, end, c, deltaT, 0.5, preset, mode)
    return model, geo, dict(walls=walls, box=box, ns=ns, start=start, end=end, c=c, deltaT=deltaT, Y=0.5)


def params_of_model(model):
    """fp32 oracle Params (leaves requiring grad) from a model with the reference's attribute names."""
    return R.Params(*[t.detach().cpu() for t in (model._mu, model._scaling, model._rotation, model._opacity,
                                                  model._features_dc, model._features_rest)],
                    int(model.active_sh_degree))
