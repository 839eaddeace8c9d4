"""float64 reference of the batched volume render and its backward, and the per-Gaussian metric the backward
is judged by (plain module, no tests; shared by test_volume_oracle_cpu.py, test_gpu_bwd_edges.py,
test_gpu_fwd_edges.py, test_gpu_ray_upstream.py and test_gpu_tile_edges.py).

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

The per-bin forward metric (forward_bins, forward_bin_failures, forward_bin_worst).  Every bin k of every wall
point p is judged by itself, not against its row's maximum:

    |hip[p, k] - ref[p, k]|  <=  sum_g tol_g (A_g + B_g)[p, k]  +  B[p, k] (1 + 1e-9)  +  Q[p, k]

    A_g[p, k] = hscale[p] att[k] sum_rays |sin(theta) val_g|   what Gaussian g puts into the bin (culled sum);
                                                               A = sum_g A_g is the bin's own scale
    B_g[p, k] = the same sum over |dense - culled| samples     what a TAIL drain may add for g outside the support:
                                                               these values are fp32 evaluations too, and in a bin
                                                               no support reaches (A = 0) they are all there is
                                                               (measured: 1e-5 to 3e-4 of themselves); 0 for the
                                                               dense and the masked forward
    tol_g     = FWD_BIN_TOL + C_FWD m_c |u0|_g U               forward_tolerance(): the fp32 position allowance
                                                               derived in test_gpu_bwd_edges.py, charged to the
                                                               Gaussian it belongs to through A_g
    B[p, k]   = |dense - ref|[p, k]                            the TAIL overrun, the unions of two rays' ranges and
                                                               the early placement bins add exact Gaussian values
                                                               outside the support, so the result lies between the
                                                               culled and the dense sum (0 for the dense and the
                                                               masked forward: FwdBins.masked())
    Q[p, k]   = 1/2 2^-E att[k] hscale[p] n[p]                 fixed-point (FX) launches only, see below
    n[p]      = the (Gaussian, ray) pairs of wall point p with a sample of m^2 <= (1.001 m_c)^2

Q.  The FX drain carries, per pair, lw = log2(w) + fxE (fxE = E = fx_info[0], w = sigma rho, netf: w c dT) and
adds log2 sin(theta) per ray, so the number a lane forms for bin k is v 2^E with v = sin(theta) val exactly the
reference's summand; it is rounded to the nearest integer (one rounding per ray and bin; a twin adds its two rays'
values first and rounds the sum once) and added, as an integer, into the u32 field / the u64 row, which is exact.
fx_reduce_kernel then returns hist[p, k] = (count 2^-E) att[k] hscale[p].  A rounding is at most half a unit, the
units of bin k are worth 2^-E att[k] hscale[p] each, and at most n[p] rays are drained for wall point p (every
drained ray has a sample inside its support; counting at 1.001 m_c keeps an fp32 mask flip from adding a ray the
count lacks: the kernel's m^2 is off by at most 2 x 40 m_c U |u0|, forward_bins asserts that this is below the
2e-3 m_c^2 the enlarged cutoff adds).  So Q bounds the rounding of the whole bin whatever the pairing, the order
or the split between the LDS and the bright launch; it is a bound, not a fit.  The unit itself: the bound of the
quantile Gaussian is below 2^kFxBits units and E never is coarser than for the largest bound, a_max in
[2^(e-1), 2^e) gives 2^-E = 2^e / 2^kFxBits <= a_max / 2^(kFxBits-1): coarsest_E().

Per-ray outputs, the per-ray upstream, occlusion and AABB selection (ray_outputs, reference(..., gray, selection),
decision_margins).  out[k, ray] is the sum over the ray's Gaussians at bin k before any table is applied:

    noocl / netf   out = sum_g val_g                              (sample_values)
    occl           D = sum_g sigma pdf,  W = sum_g rho (1 - exp(-sigma pdf c dT)),
                   T_k = exp(-c dT sum_{k' < k} D_k'),  out_k = T_k W_k if T_k >= 1e-4 else 0
                   (oracle.torch_ref.render_rays_cuda(use_occlusion=True) in double; cuda preset)
    rays[p, i np + j, k] = ray_scale out[k, ray]                  render_forward(want_rays=True)
    hist[p, k]           = hscale[p] att[k] sum_rays sin(theta) out[k, ray]

selection="aabb" keeps, per ray, the first 256 Gaussians by index whose box (`boxes` [Ng, 6]: nlosgr.render.bboxes,
or oracle.torch_ref.bboxes_cuda) the half-infinite ray hits (oracle.torch_ref.aabb_filter's slab test in double);
the list is an input of the arithmetic, not part of it.  A selected Gaussian is evaluated over the whole ray, or
within the cutoff when one is set.  reference(..., gout, gray) returns the gradient of sum(hist gout) + sum(rays
gray); either upstream may be None, and the sign split behind s_g and b_g takes the positive parts of both, then
the negative parts of both.  Three decisions are discontinuous (T >= 1e-4, the slab test, the 256 cap);
decision_margins() measures how far a scene stays from the first two, and the tests that use a scene assert 1e-3.

FWD_BIN_TOL is 2e-5, the row tolerance it replaces.  The worst (e - B - Q)^+ / (A + sum_g B_g) measured on the
MI355X over the well-conditioned scenes (1, 4, 5 of tests/test_gpu_fwd_edges.py) and all their variants is 1.6e-5;
four times that would pass 2e-5, which is traced in that file's docstring to the exp2 recurrence of the drains and
left at 2e-5.  The measured table is there and in DESIGN.md section 7.
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


CAP = 256   # AABB selection: Gaussians per ray (ray_aabb.cu)


def slab_times(tab, p, boxes):
    """(tmin, tmax) [rays, Ng] float64 of oracle.torch_ref.aabb_filter's slab test for the rays of wall point p:
    a ray selects a box iff tmax >= tmin and tmax >= 0."""
    d, _ = directions(tab, p)
    bb = boxes.detach().cpu().double()
    o = tab["wall"][p]
    inv = 1.0 / (d + 1e-8)
    t0 = (bb[None, :, 0:3] - o[None, None, :]) * inv[:, None, :]
    t1 = (bb[None, :, 3:6] - o[None, None, :]) * inv[:, None, :]
    return torch.minimum(t0, t1).amax(-1), torch.maximum(t0, t1).amin(-1)


def selection_mask(tab, p, boxes, cap=CAP):
    """bool [Ng, rays]: the Gaussians each ray of wall point p selects (the first `cap` hits by index)."""
    tmin, tmax = slab_times(tab, p, boxes)
    hit = (tmax >= tmin) & (tmax >= 0)
    return (hit & (torch.cumsum(hit.long(), dim=1) <= cap)).t().contiguous()


def ray_outputs(P, tab, p, preset, mode, c_deltaT, cutoff, sel=None):
    """out [nr, rays] (float64, differentiable in P's leaves; module docstring) and, for occl, T [nr, rays] as the
    exclusive product continues it (not zeroed past the cut; None otherwise).  sel: selection_mask or None."""
    if mode in ("noocl", "netf"):
        v = sample_values(P, tab, p, preset, mode, c_deltaT, cutoff)
        if sel is not None:
            v = v * sel[:, None, :].double()
        return v.sum(dim=0), None
    if mode != "occl" or preset != "cuda":
        raise ValueError((preset, mode))
    x, _ = _points(tab, p)
    nr, nray = x.shape[0], x.shape[1]
    ng = P._mu.shape[0]
    pdf = R.gaussian_pdf(x.reshape(-1, 3), P, preset, 1.0, _mc(cutoff)).view(ng, nr, nray)
    if sel is not None:
        pdf = pdf * sel[:, None, :].double()
    sig = torch.sigmoid(P._opacity).reshape(ng, 1, 1)
    rho = R.albedo(P, tab["wall"][p], preset).reshape(ng, 1, 1)
    c = sig * pdf
    D = c.sum(dim=0)
    W = (-torch.expm1(-c * c_deltaT) * rho).sum(dim=0)
    tau = torch.cumsum(D, dim=0) - D                      # exclusive
    T = torch.exp(-c_deltaT * tau)
    live = (T >= 1e-4).double()
    return T * W * live, T


def _up(t):
    return None if t is None else t.detach().cpu().double()


def _split_grads(P, tab, preset, mode, c_deltaT, cutoff, gout, culled=None, gray=None, sels=None, ray_scale=1.0):
    """hist [P, nr], rays [P, rays, nr] and, per tensor, G [P, 2, Ng, C]: the gradient of sum(hist gout) +
    sum(rays gray) under the positive / the negative parts of both upstreams."""
    nw = tab["wall"].shape[0]
    hist, rays, G = [], [], {n: [] for n in NAMES}
    for p in range(nw):
        if culled is not None and _mc(cutoff) is not None:
            with torch.no_grad():
                x, _ = _points(tab, p)
                culled.append(int((R.gaussian_pdf(x.reshape(-1, 3), P, preset, 1.0, _mc(cutoff)) == 0).sum()))
        out, _ = ray_outputs(P, tab, p, preset, mode, c_deltaT, cutoff, None if sels is None else sels[p])
        w = directions(tab, p)[1]
        fold = tab["hscale"][p] * tab["att"][:, None] * w[None, :]          # [nr, rays]: d hist[k] / d out[k, ray]
        hist.append((fold * out).sum(dim=1).detach())
        rays.append((ray_scale * out.t()).detach())
        rows = []
        for s in (1.0, -1.0):
            up = torch.zeros_like(out)
            if gout is not None:
                up = up + fold * torch.clamp_min(s * gout[p], 0.0)[:, None]
            if gray is not None:
                up = up + ray_scale * torch.clamp_min(s * gray[p], 0.0).t()
            rows.append(torch.autograd.grad(out, P.leaves(), grad_outputs=up, retain_graph=(s > 0), allow_unused=True))
        for i, n in enumerate(NAMES):
            z = torch.zeros_like(P.leaves()[i])
            G[n].append(torch.stack([(r[i] if r[i] is not None else z).reshape(z.shape[0], -1) for r in rows]))
    return torch.stack(hist), torch.stack(rays), {n: torch.stack(v) for n, v in G.items()}


@dataclass
class Reference:
    hist: torch.Tensor          # [P, nr]
    hist_bracket: torch.Tensor  # [P]   max_k |dense - culled|
    grads: dict                 # name -> [Ng, C]
    scale: dict                 # name -> [Ng]   s_g
    bracket: dict               # name -> [Ng]   b_g
    rays: torch.Tensor = None          # [P, rays, nr]   ray_scale out
    rays_bracket: torch.Tensor = None  # [P, rays, nr]   |dense - culled| per sample


def _selections(tab, selection, boxes):
    if selection == "support":
        return None
    if selection != "aabb" or boxes is None:
        raise ValueError("selection is 'support' or 'aabb' (with boxes [Ng, 6])")
    with torch.no_grad():
        return [selection_mask(tab, p, boxes) for p in range(tab["wall"].shape[0])]


def reference(P, geo, preset, mode, c_deltaT, cutoff, gout, gray=None, selection="support", boxes=None,
              ray_scale=1.0):
    """The float64 forward (hist and rays), the gradient of sum(hist gout) + sum(rays gray) (gout [P, nr], gray
    [P, nt * np, nr]; either may be None), and the metric's s_g and b_g."""
    tab = tables(geo)
    P = Params64(P)
    gout, gray = _up(gout), _up(gray)
    sels = _selections(tab, selection, boxes)
    culled = []
    kw = dict(gray=gray, sels=sels, ray_scale=float(ray_scale))
    hist, rays, G = _split_grads(P, tab, preset, mode, c_deltaT, cutoff, gout, culled, **kw)
    grads = {n: (g[:, 0] - g[:, 1]).sum(0) for n, g in G.items()}
    scale = {n: _rowmax(g).sum(dim=(0, 1)) for n, g in G.items()}
    if _mc(cutoff) is None or sum(culled) == 0:   # nothing culled: the dense reference is the same sum
        bracket = {n: torch.zeros_like(scale[n]) for n in NAMES}
        hb = torch.zeros(hist.shape[0], dtype=hist.dtype)
        rb = torch.zeros_like(rays)
    else:
        dh, dr, DG = _split_grads(P, tab, preset, mode, c_deltaT, None, gout, **kw)
        bracket = {n: _rowmax(DG[n] - G[n]).sum(dim=(0, 1)) for n in NAMES}
        hb = (dh - hist).abs().amax(dim=1)
        rb = (dr - rays).abs()
    return Reference(hist, hb, grads, scale, bracket, rays, rb)


def forward_rays(P, geo, preset, mode, c_deltaT, cutoff, selection="support", boxes=None, ray_scale=1.0):
    """(hist [P, nr], rays [P, rays, nr], T [P, nr, rays] or None, sels) in float64, no graph."""
    tab = tables(geo)
    P = Params64(P)
    sels = _selections(tab, selection, boxes)
    hist, rays, Ts = [], [], []
    with torch.no_grad():
        for p in range(tab["wall"].shape[0]):
            out, T = ray_outputs(P, tab, p, preset, mode, c_deltaT, cutoff, None if sels is None else sels[p])
            w = directions(tab, p)[1]
            hist.append(tab["hscale"][p] * tab["att"] * (out * w[None, :]).sum(dim=1))
            rays.append(ray_scale * out.t())
            Ts.append(T)
    return torch.stack(hist), torch.stack(rays), (torch.stack(Ts) if Ts[0] is not None else None), sels


def decision_margins(P, geo, preset, mode, c_deltaT, cutoff, selection="support", boxes=None):
    """How far the scene stays from the model's discontinuous decisions, in float64:
        "T"     the smallest |T_k / 1e-4 - 1| over every sample, live or dead (inf without occlusion)
        "slab"  the smallest of |tmax - tmin| and |tmax| over every (ray, box), over the ray's length r[nr - 1]
                (inf under support selection)
    The tests assert both above 1e-3: fp32 moves T by 1e-5 relative at most (an exponent below 10 summed in
    fp32) and a slab time by 1e-6."""
    tab = tables(geo)
    out = {"T": float("inf"), "slab": float("inf")}
    if mode == "occl":
        T = forward_rays(P, geo, preset, mode, c_deltaT, cutoff, selection, boxes)[2]
        out["T"] = float((T / 1e-4 - 1.0).abs().min())
    if selection == "aabb":
        length = float(tab["r"][-1])
        for p in range(tab["wall"].shape[0]):
            tmin, tmax = slab_times(tab, p, boxes)
            out["slab"] = min(out["slab"], float((tmax - tmin).abs().min()) / length, float(tmax.abs().min()) / length)
    return out


def rays_worst(rays, ref, absolute=None):
    """The smallest constant c with |rays - ref| <= c |ref| + bracket + absolute for every (ray, bin): max of
    (e - bracket - absolute)^+ / |ref| (inf where ref = 0 and the sample is beyond its allowances: a dead sample
    must come out exactly zero)."""
    e = (rays.detach().cpu().double().reshape(ref.rays.shape) - ref.rays).abs()
    x = torch.clamp_min(e - ref.rays_bracket * (1 + 1e-9) - (0.0 if absolute is None else absolute), 0.0)
    a = ref.rays.abs()
    rel = torch.where(a > 0, x / a.clamp_min(1e-300), torch.where(x > 0, torch.full_like(x, float("inf")),
                                                                   torch.zeros_like(x)))
    return float(rel.max()) if rel.numel() else 0.0


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
# the forward, bin by bin (module docstring)
# --------------------------------------------------------------------------------------------
U = 2.0 ** -24          # fp32 unit roundoff
C_FWD = 32.0            # the forward's position allowance C_FWD m_c |u0| U (derived in test_gpu_bwd_edges.py)
FX_BITS = 24            # kFxBits of csrc/nlosgr_volume_fwd.hip
# Four times the worst per-bin value measured on the MI355X over scenes 1, 4 and 5 of test_gpu_fwd_edges.py (1.6e-5,
# table in that file) would be 7e-5; the constant stays at 2e-5, the row tolerance it replaces, which leaves a margin
# of 1.25 instead of 4.  The excess is traced to the drains' exp2 recurrence (that file's docstring), not fixed here.
FWD_BIN_TOL = 2e-5
assert FWD_BIN_TOL <= 2e-5


def sample_values(P, tab, p, preset, mode, c_deltaT, cutoff):
    """[Ng, nr, rays] float64: val_g of every sample of wall point p (0 outside the support): what the per-sample
    output rays[p, ray, k] sums over the Gaussians (times ray_scale).  P: Params64 (or float64 Params)."""
    x, _ = _points(tab, p)
    nr, nray = x.shape[0], x.shape[1]
    ng = P._mu.shape[0]
    pdf = R.gaussian_pdf(x.reshape(-1, 3), P, preset, 1.0, _mc(cutoff)).view(ng, nr, nray)
    sig = torch.sigmoid(P._opacity).reshape(ng, 1, 1)
    rho = R.albedo(P, tab["wall"][p], preset).reshape(ng, 1, 1)
    if mode == "noocl":
        return sig * rho * pdf
    if mode == "netf":
        D = sig * pdf
        f = torch.exp(-D * c_deltaT) + 1e-7
        T = torch.cat([torch.ones_like(f[:, :1]), torch.cumprod(f, dim=1)[:, :-1]], dim=1)
        return D * T * rho * c_deltaT
    raise ValueError(mode)


def ray_terms(P, tab, p, preset, mode, c_deltaT, cutoff):
    """[Ng, nr, rays] float64: hscale[p] att[k] sin(theta) val_g of every sample of wall point p (0 outside the
    support), so that hist[p, k] is its sum over Gaussians and rays."""
    _, w = _points(tab, p)
    return tab["hscale"][p] * tab["att"][None, :, None] * sample_values(P, tab, p, preset, mode, c_deltaT, cutoff) \
        * w[None, None, :]


def edge_band(P, tab, p, preset, cutoff, rel=2e-3):
    """bool [Ng, nr, rays]: the samples whose m^2 is within rel of cutoff^2, where an fp32 evaluation of m^2 may
    put the sample on the other side of the mask (the kernel's m^2 is off by at most 80 m_c U |u0|: forward_bins)."""
    x, _ = _points(tab, p)
    m2 = -2.0 * torch.log(R.gaussian_pdf(x.reshape(-1, 3), P, preset, 1.0, None).clamp_min(1e-300))
    mc2 = float(cutoff) ** 2
    return ((m2 - mc2).abs() <= rel * mc2).view(P._mu.shape[0], x.shape[0], x.shape[1])


@dataclass
class FwdBins:
    ref: torch.Tensor      # [P, nr]      the culled sum
    dense: torch.Tensor    # [P, nr]      the dense sum
    A_g: torch.Tensor      # [P, Ng, nr]  hscale att sum_rays |sin(theta) val_g|
    B_g: torch.Tensor      # [P, Ng, nr]  hscale att sum_rays |sin(theta) (val_g dense - val_g culled)|
    n: torch.Tensor        # [P]          (Gaussian, ray) pairs with a sample inside 1.001 m_c
    unit: torch.Tensor     # [P, nr]      att[k] hscale[p]: what one count of 2^-E is worth in bin k, over 2^-E

    @property
    def A(self):
        return self.A_g.sum(dim=1)

    @property
    def B(self):
        return (self.dense - self.ref).abs()

    @property
    def S(self):
        """[P, nr]: everything a drain may add to the bin, the scale of its fp32 error: A plus the out-of-support
        values (A for the dense and the masked forward)."""
        return (self.A_g + self.B_g).sum(dim=1)

    def Q(self, E):
        """[P, nr]: the FX rounding bound at unit 2^-E (zeros for E None: a float drain)."""
        if E is None:
            return torch.zeros_like(self.ref)
        return 0.5 * 2.0 ** (-float(E)) * self.unit * self.n[:, None]

    def masked(self):
        """The same reference for a forward that adds nothing outside the support (FLAG_MASKED_FWD): B = 0."""
        return FwdBins(self.ref, self.ref, self.A_g, torch.zeros_like(self.B_g), self.n, self.unit)


def forward_bins(P, geo, preset, mode, c_deltaT, cutoff):
    """The float64 forward of a scene bin by bin: FwdBins (module docstring)."""
    tab = tables(geo)
    P = Params64(P)
    mc = _mc(cutoff)
    if mc is not None:
        # the count's enlarged cutoff must cover the kernel's fp32 position error: m^2 / 2 moves by at most
        # 40 m_c U |u0| (test_gpu_bwd_edges.py), m^2 by twice that, against the (1.001^2 - 1) m_c^2 of the wider cutoff
        u0, _ = conditioning(P, geo, preset)
        assert 2 * 40.0 * mc * U * float(u0.max()) < (1.001 ** 2 - 1.0) * mc * mc, ("|u0| too large for the ray count",
                                                                                    float(u0.max()))
    ref, dense, A_g, B_g, n = [], [], [], [], []
    with torch.no_grad():
        for p in range(tab["wall"].shape[0]):
            t = ray_terms(P, tab, p, preset, mode, c_deltaT, cutoff)
            ref.append(t.sum(dim=(0, 2)))
            A_g.append(t.abs().sum(dim=2))
            if mc is None:
                dense.append(ref[-1])
                B_g.append(torch.zeros_like(A_g[-1]))
                n.append(t.shape[0] * t.shape[2])
            else:
                td = ray_terms(P, tab, p, preset, mode, c_deltaT, None)
                dense.append(td.sum(dim=(0, 2)))
                B_g.append((td - t).abs().sum(dim=2))
                x, _ = _points(tab, p)
                wide = R.gaussian_pdf(x.reshape(-1, 3), P, preset, 1.0, 1.001 * mc).view(t.shape) > 0
                n.append(int(wide.any(dim=1).sum()))
    unit = tab["hscale"][:, None] * tab["att"][None, :]
    return FwdBins(torch.stack(ref), torch.stack(dense), torch.stack(A_g), torch.stack(B_g),
                   torch.tensor(n, dtype=torch.float64), unit)


def forward_tolerance(P, geo, preset, cutoff, base=None):
    """tol_g [Ng] = base (FWD_BIN_TOL) + C_FWD m_c |u0|_g U, from the scene alone."""
    u0, _ = conditioning(P, geo, preset)
    return (FWD_BIN_TOL if base is None else base) + C_FWD * max(float(cutoff), 1.0) * u0 * U


def fx_bound(P, preset, mode, c_deltaT):
    """[Ng] float64: the amplitude bound sigma rho_max of fx_bound_kernel (rho_max by Cauchy-Schwarz over the SH
    bands, with the kernel's 5 % and 0.1 % margins; netf: times c dT)."""
    P = Params64(P)
    with torch.no_grad():
        f = P.features[:, :, 0]
        deg = min(int(P.active_sh_degree), 4 if preset == "torch" else 3)
        sh = sum(f[:, l * l:(l + 1) * (l + 1)].norm(dim=1) * ((2 * l + 1) / (4 * torch.pi)) ** 0.5
                 for l in range(deg + 1) if l * l < f.shape[1])
        return torch.sigmoid(P._opacity).reshape(-1) * (0.5 + 1.05 * sh) * 1.001 * (c_deltaT if mode == "netf" else 1.0)


def coarsest_E(P, preset, mode, c_deltaT):
    """The coarsest unit exponent the quantile rule can pick for a scene, as a real number: the unit never
    exceeds the largest bound over 2^(FX_BITS - 1) (module docstring).  A launch's fx_info E is >= this."""
    import math
    return (FX_BITS - 1) - math.log2(float(fx_bound(P, preset, mode, c_deltaT).max()))


def quantile_E(P, preset, mode, c_deltaT, nrays):
    """(E, E of the largest bound) as fx_unit_kernel picks them from the bounds' binary exponents: the unit of the
    ceil(ng / 256)-th brightest bound, at most `range` binary orders finer than the largest bound's (run_fwd:
    range = 63 - FX_BITS - ceil(log2(ceil(ng / 256) nrays)), at most 16).  A bound within an fp32 rounding of a
    power of two could fall on the other side in the kernel."""
    import math
    b = fx_bound(P, preset, mode, c_deltaT)
    b = b[(b > 0) & (b < 3.0e38)]
    if b.numel() == 0:
        return 0, 0
    e = torch.floor(torch.log2(b)).long() + 1            # b in [2^(e-1), 2^e): E = FX_BITS - e
    kq = (b.numel() + 255) // 256
    eq, et = int(e.sort(descending=True).values[kq - 1]), int(e.max())
    bits = max(0, math.ceil(math.log2(max(((int(P._mu.shape[0]) + 255) // 256) * nrays, 1))))
    rng = min(max(63 - FX_BITS - bits, 0), 16)
    return min(FX_BITS - eq, FX_BITS - et + rng), FX_BITS - et


def _bin_bound(ref, tol, E):
    t = tol.double() if torch.is_tensor(tol) else torch.full((ref.A_g.shape[1],), float(tol), dtype=torch.float64)
    # (2^-126: what lies below the smallest normal fp32 number, before or after the factor att hscale, is not resolved:
    # a bin holding only the far tail of one Gaussian comes out as a multiple of 2^-149)
    return (torch.einsum("g,pgk->pk", t, ref.A_g + ref.B_g), ref.B * (1 + 1e-9) + 2.0 ** -126 * ref.unit.clamp_min(1.0),
            ref.Q(E))


def forward_bin_failures(hist, ref, tol, E=None):
    """[(p, k, e, tol part, B, Q)] of every bin with e = |hist - ref| > sum_g tol_g (A_g + B_g) + B (1 + 1e-9) + Q.
    tol: one number or [Ng]; E: the launch's fx_info E (None for a float drain: Q = 0).  Bins with A = 0 must
    come out within B + Q, up to the fp32 error of the out-of-support values themselves (tol_g B_g)."""
    e = (hist.detach().cpu().double() - ref.ref).abs()
    ta, b, q = _bin_bound(ref, tol, E)
    bad = torch.nonzero(~(e <= ta + b + q))   # (a NaN fails)
    return [(int(p), int(k), float(e[p, k]), float(ta[p, k]), float(b[p, k]), float(q[p, k])) for p, k in bad]


def forward_bin_excess(hist, ref, E=None):
    """[P, nr]: (e - B - Q)^+ / S, the smallest uniform tol each bin passes with (S = A plus the out-of-support
    values a TAIL drain may add; inf where S = 0 and the bin is beyond B + Q)."""
    e = (hist.detach().cpu().double() - ref.ref).abs()
    _, b, q = _bin_bound(ref, 0.0, E)
    x, A = torch.clamp_min(e - b - q, 0.0), ref.S
    return torch.where(A > 0, x / A.clamp_min(1e-300), torch.where(x > 0, torch.full_like(x, float("inf")),
                                                                   torch.zeros_like(x)))


def forward_bin_worst(hist, ref, E=None):
    """The smallest uniform tol that passes every bin: max over bins of (e - B - Q)^+ / S."""
    return float(forward_bin_excess(hist, ref, E).max())


def forward_bin_coverage(ref, tol, E):
    """Of the bins with ref > 0, the fraction in which the bracket or the rounding decides: B + Q > 10 sum_g
    tol_g (A_g + B_g)."""
    ta, b, q = _bin_bound(ref, tol, E)
    live = ref.ref > 0
    return float(((b + q > 10.0 * ta) & live).sum()) / max(int(live.sum()), 1)


def as_row_reference(fb):
    """A FwdBins as forward_worst() takes its reference (hist and the row bracket max_k |dense - culled|)."""
    return Reference(fb.ref, fb.B.amax(dim=1), {}, {}, {})


# --------------------------------------------------------------------------------------------
# scenes shared by the CPU and the GPU tests
# --------------------------------------------------------------------------------------------
def parity_scene(preset, mode, T, device=None, scale_shift=None, ng=48, ns=6, wall=(2, 3), seed=3, edit=None,
                 start=None, deltaT=None):
    """The scene of tests/test_gpu_parity.py::_volume_vs_oracle: `ng` synthetic Gaussians of SH degree 3 (cuda
    preset: log-scales + 1.2, or + scale_shift), a 2 x 3 relay wall, ns x ns rays, T bins of 1.28 / T from bin
    T // 8 (or of `deltaT` from bin `start`).  edit(model, walls) may change the parameters in place.  Returns
    (model, geo, consts) with consts =
    dict(walls, box, ns, start, end, c, deltaT, Y) as oracle.torch_ref.render_volume takes them."""
    from nlosgr import GaussianParams
    from nlosgr.geometry import build_geometry, relay_wall_grid, volume_box_point
    c, deltaT = 1.0, (1.28 / T if deltaT is None else deltaT)
    start = T // 8 if start is None else start
    end = start + T
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


def compact_scene(preset="cuda", mode="noocl", device=None, T=97, ns=6):
    """Scene 1 with fewer Gaussians per bin (cuda preset log-scales + 0: standard deviations about 0.14, 17 bins) and
    97 bins of 8e-3 from r = 0.24 to 1.008, which end inside the hidden volume: rows with structure, segments that
    end inside the row and segments cut by its last bin.  |u0| <= 9: still well-conditioned."""
    return parity_scene(preset, mode, T, device, scale_shift=0.0, ns=ns, start=30, deltaT=8e-3)


def _rand_log(g, n, lo, hi):
    import math
    return math.log(lo) + (math.log(hi) - math.log(lo)) * torch.rand(n, generator=g)


def runs_scene(ns, device=None, mode="noocl", ng=64, T=97, wall=(1, 3), seed=41, sigma=(0.035, 0.11), edit=None):
    """Scene 4 of test_gpu_fwd_edges.py (cuda preset): `ng` Gaussians of standard deviation sigma[0] ..
    sigma[1] (log-uniform, axes within 20 %), centred anywhere in a slab 1.6 times as wide as the hidden volume,
    so that many 5.7-sigma boxes are cut by the edge of the ray grid: their rows hold runs of 1 .. ns passing
    cells, some ending with the row.  Albedo about 0.4 (never clamped).  edit(model, walls) may change them."""
    def place(m, walls):
        g = torch.Generator().manual_seed(seed)
        n = m._mu.shape[0]
        mu = torch.tensor([0.0, 0.5, 0.0]) + (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([0.8, 0.5, 0.8])
        s = _rand_log(g, n, *sigma)[:, None] + 0.2 * (torch.rand(n, 3, generator=g) - 0.5)
        dev = m._mu.device
        m._mu[:] = mu.float().to(dev)
        m._scaling[:] = s.float().to(dev)
        m._features_dc[:] = (0.4 - 0.5) / R.C0
        if edit is not None:
            edit(m, walls)
    return parity_scene("cuda", mode, T, device, ng=ng, ns=ns, wall=wall, seed=seed, edit=place)


def run_lengths(model, geo, cutoff):
    """Per wall point, the lengths of the runs of passing cells in the rows of every pair's box, and whether a
    run ends with its row of the ray grid (float64 replay of the enumeration, nlosgr.enum_replay); also the
    number of pairs the run-following scheme forms.  Returns (sorted set of lengths, runs ending with the row,
    pairs)."""
    import numpy as np
    from nlosgr import enum_replay as E
    cpu = lambda t: t.detach().cpu()
    Pm = params_of_model(model)
    mu = cpu(model._mu).numpy().astype(np.float64)
    A, smax = E.gaussian_frames(mu, cpu(model._scaling).numpy(), cpu(model._rotation).numpy())
    lengths, at_end, pairs = set(), 0, 0
    for p in range(geo.nwall):
        box, ok, _, _ = E.wall_point_cells(geo, p, mu, A, smax, cutoff)
        rho = R.albedo(Pm, cpu(geo.wall[p]).float(), preset="cuda")[:, 0].detach().numpy()
        ok &= (rho > 0)[:, None, None]
        for g in np.nonzero(ok.any((1, 2)))[0]:
            i0, i1, j0, j1 = box[g]
            okb = ok[g, i0:i1 + 1, j0:j1 + 1]
            pairs += sum(l == 2 for _, _, l in E.groups_run(okb, 2)[0])
            for row in okb:
                run = 0
                for c, v in enumerate(list(row) + [False]):
                    if v:
                        run += 1
                    elif run:
                        lengths.add(run)
                        at_end += int(j0 + c == geo.np)
                        run = 0
    return sorted(lengths), at_end, pairs


def lane_boundary(ng):
    """The Gaussians either side of every 64-Gaussian boundary (a wave's chunk; the forward's Gaussian splits start
    on multiples of 64) and the last one: bool [ng]."""
    i = torch.arange(ng)
    return (i % 64 == 0) | (i % 64 == 63) | (i == ng - 1)


def lanes_scene(ng, nwall, device=None, mode="noocl", T=49, ns=6, seed=51, sigma=0.08, deltaT=0.015, start=17):
    """Scene 5 of test_gpu_fwd_edges.py (cuda preset): `ng` Gaussians of standard deviation 0.08 (axes within
    20 %, 5.3 bins; 49 bins of 0.015 from r = 0.255 to 0.975, c dT <= 1/64) whose centres are spread evenly over
    the ranges the rows cover, in a random order
    of the index, so that the Gaussians that dominate a bin change from bin to bin and with the wall point.  Above
    65 Gaussians a bin holds too many for every one to stand out, so all but those at the chunk boundaries
    (lane_boundary) are dimmed (opacity - 5: about 1 / 100)."""
    import math

    def edit(m, walls):
        g = torch.Generator().manual_seed(seed + ng)
        n = m._mu.shape[0]
        r = 0.3 + 0.65 * (torch.randperm(n, generator=g).double() + 0.5) / n        # distance from the wall's centre
        th = 0.35 * (torch.rand(n, generator=g).double() - 0.5)                      # a narrow fan about +y
        ph = 0.35 * (torch.rand(n, generator=g).double() - 0.5)
        mu = torch.stack([r * torch.sin(th), r * torch.cos(th) * torch.cos(ph), r * torch.cos(th) * torch.sin(ph)], 1)
        dev = m._mu.device
        m._mu[:] = mu.float().to(dev)
        m._scaling[:] = (math.log(sigma) + 0.2 * (torch.rand(n, 3, generator=g) - 0.5)).float().to(dev)
        m._features_dc[:] = (0.4 - 0.5) / R.C0
        m._opacity[:] = 0.5 * torch.randn(n, 1, generator=g).to(dev)
        if n > 65:
            m._opacity[~lane_boundary(n).to(dev)] -= 5.0
    return parity_scene("cuda", mode, T, device, ng=ng, ns=ns, wall=(1, nwall), seed=seed, edit=edit, start=start,
                        deltaT=deltaT)


def pile_scene(device=None, ng=128, T=97, ns=12, seed=71):
    """The flush case of scene 7: `ng` co-located, equally bright, wide Gaussians (opacity 4, albedo 1, no SH rest,
    sigma 0.1 at the volume's centre: tests/test_gpu_fx.py's pile, smaller).  None is brighter than the quantile,
    every ray peaks within a few bins at up to 2^23 units, and a wave drains 64 x ns^2 of them at a time into one
    LDS histogram: its fields pass 2^31 and are moved to the u64 row."""
    import math

    def edit(m, walls):
        g = torch.Generator().manual_seed(seed)
        n = m._mu.shape[0]
        dev = m._mu.device
        m._mu[:] = (torch.tensor([0.0, 0.5, 0.0]) + 1e-3 * torch.randn(n, 3, generator=g)).float().to(dev)
        m._scaling[:] = (math.log(0.1) + 0.05 * torch.randn(n, 3, generator=g)).float().to(dev)
        m._opacity[:] = 4.0
        m._features_dc[:] = (1.0 - 0.5) / R.C0
        m._features_rest[:] = 0.0
    return parity_scene("cuda", "noocl", T, device, ng=ng, ns=ns, wall=(1, 2), seed=seed, edit=edit, start=20,
                        deltaT=8e-3)


def bright_scene(nbright, device=None, mode="noocl", ng=300, T=97, ns=8, seed=61):
    """Scene 7 of test_gpu_fwd_edges.py (cuda preset): 300 Gaussians (the quantile of the FX unit is the second
    brightest bound), the first `nbright` of them about 4000 times brighter (opacity 4, albedo 200, no SH rest:
    tests/test_gpu_fx.py) and small (sigma 0.03), so that most bins are out of their reach."""
    import math

    def edit(m, walls):
        if nbright:
            m._opacity[:nbright] = 4.0
            m._features_dc[:nbright] = (200.0 - 0.5) / R.C0
            m._features_rest[:nbright] = 0.0
            m._scaling[:nbright] = math.log(0.03)
    return parity_scene("cuda", mode, T, device, ng=ng, ns=ns, wall=(1, 2), seed=seed, edit=edit)


def tight_albedo(m, opacity=2.0):
    """Every Gaussian equally bright with an albedo its amplitude bound is tight for (opacity 2: sigma 0.88, albedo 1,
    no SH rest: bound 1.03 sigma), so that the FX unit, set from the largest bound, is as fine as the scene allows:
    in scenes of thin Gaussians many bins hold only flank samples, and the rounding bound Q is what they compete
    with."""
    m._opacity[:] = opacity
    m._features_dc[:] = (1.0 - 0.5) / R.C0
    m._features_rest[:] = 0.0


def params_of_model(model):
    """fp32 oracle Params (leaves requiring grad) from a model with the reference's attribute names."""
    return R.Params(*[t.detach().cpu() for t in (model._mu, model._scaling, model._rotation, model._opacity,
                                                  model._features_dc, model._features_rest)],
                    int(model.active_sh_degree))


# --------------------------------------------------------------------------------------------
# scenes of test_gpu_ray_upstream.py and test_gpu_tile_edges.py
# --------------------------------------------------------------------------------------------
def ranges_geometry(walls, box, nt, nphi, start, end, c, deltaT, Y, preset, mode):
    """nlosgr.geometry.build_geometry with nt != np (geometry_from_ranges over the same angular ranges)."""
    from nlosgr.geometry import angle_ranges, geometry_from_ranges, radial_tables
    walls = walls.float().contiguous()
    tmin, tmax, pmin, pmax = angle_ranges(walls, box.to(walls.device).float())
    extra = float(Y) ** 2 * (c * deltaT if preset == "cuda" and mode in ("noocl", "binint") else 1.0)
    r, att, _, _ = radial_tables(start, end, c, deltaT, preset, walls.device)
    return geometry_from_ranges(walls, tmin, tmax, pmin, pmax, nt, nphi, r, att, extra)


UPSTREAM_SHAPES = {            # name -> (T, wall, nt, np, compact)
    "T41-1x3-7x4": (41, (1, 3), 7, 4, False),     # c dT > 1/64: the netf exp path
    "T97-2x3-4x7": (97, (2, 3), 4, 7, True),      # c dT = 8e-3: the exp-free path; supports end inside the rows
    "T97-1x3-6x6": (97, (1, 3), 6, 6, False),
}


def upstream_scene(preset, mode, shape, device=None):
    """The pair-major scenes of test_gpu_ray_upstream.py: parity_scene's 48 Gaussians (compact: compact_scene's,
    narrower, on 97 bins of 8e-3 from r = 0.24) over nt x np rays with nt != np.  Returns (model, geo, consts)."""
    T, wall, nt, nphi, compact = UPSTREAM_SHAPES[shape]
    kw = dict(scale_shift=0.0, start=30, deltaT=8e-3) if compact else {}
    model, _, k = parity_scene(preset, mode, T, device, wall=wall, **kw)
    geo = ranges_geometry(k["walls"], k["box"], nt, nphi, k["start"], k["end"], k["c"], k["deltaT"], k["Y"], preset, mode)
    return model, geo, k


def tile_scene(nr, ng, device=None, mode="occl", nt=9, nphi=5, wall=(1, 2), deg=2, seed=7, scale_shift=1.2,
               opac_shift=1.5, c_deltaT=None, edit=None, start=None):
    """The ray-tile engine's scenes (cuda preset): `ng` synthetic Gaussians of SH degree `deg` (log-scales +
    scale_shift, opacities + opac_shift: tests/test_gpu_occl.py's), nt x np rays, nr bins of c dT = 1.28 / nr (or
    c_deltaT) from bin nr // 8.  nt = 9, np = 5 leaves every tile shape of the ladder (8x8, 8x4, 4x4, 4x2, 2x2)
    tiles cut by the grid's edge in i, in j and in both.  Returns (model, geo, c dT)."""
    from nlosgr import GaussianParams
    from nlosgr.geometry import relay_wall_grid, volume_box_point
    cdt = 1.28 / nr if c_deltaT is None else float(c_deltaT)
    model = GaussianParams.synthetic(ng, deg, preset="cuda", device=device, seed=seed)
    walls = relay_wall_grid(wall[0], wall[1], device=device)
    with torch.no_grad():
        model._scaling.add_(scale_shift)
        model._opacity.add_(opac_shift)
        if edit is not None:
            edit(model, walls)
    box = volume_box_point((0.0, 0.5, 0.0), 0.5, device)
    start = nr // 8 if start is None else start
    geo = ranges_geometry(walls, box, nt, nphi, start, start + nr, 1.0, cdt, 0.5, "cuda", mode)
    return model, geo, cdt


LADDER = {40: 24, 65: 24, 257: 16, 513: 12, 1025: 10, 2049: 8, 4096: 8}   # nr -> ng (rt = 64, 64, 32, 16, 8, 4, 4)
# seeds that keep every T_k and slab time of the scene 1e-3 away from its decision (decision_margins; proven on the
# CPU by test_volume_oracle_cpu.py).  From nr = 257 on the support scenes are less opaque (T >= 4e-4 throughout): a
# scene that crosses 1e-4 with 23 000 samples of T spread over 18 e-folds has one within 1e-3 almost surely; the
# crossing at several chunks is opaque_scene's subject.
LADDER_SEED = {"support": {40: 9, 65: 20, 257: 7, 513: 7, 1025: 7, 2049: 7, 4096: 7},
               "aabb": {40: 25, 65: 25, 257: 23, 513: 8, 1025: 7, 2049: 7, 4096: 7}}


def ladder_scene(nr, device=None, mode="occl", selection="support", seed=None):
    """Part 1 of test_gpu_tile_edges.py: tile_scene at every step of tile_rays()'s ladder, 8 to 24 Gaussians: broad
    ones (standard deviation about 0.6, every sample inside 5.7 sigma) under support selection, and of about 0.2
    under AABB selection, where the 3-sigma boxes then leave out part of the rays."""
    return tile_scene(nr, LADDER[nr], device, mode, seed=LADDER_SEED[selection][nr] if seed is None else seed,
                      scale_shift=1.2 if selection == "support" else -0.5, opac_shift=1.5 if nr <= 65 else 0.0)


OPAQUE_SEED = {97: 197, 257: 358}    # proven by decision_margins on the CPU, like LADDER_SEED


def opaque_scene(nr, device=None, seed=None):
    """Part 2 of test_gpu_tile_edges.py: two blobs of 100 nearly opaque Gaussians each, one at 0.1 and one at 0.7 of
    the rays' range (nr = 97: c dT = 1/60, the exp path; nr = 257: c dT = 1/256, the polynomial), off the volume's
    axis on opposite sides: rays through the near blob lose their light (T < 1e-4) in chunk 0, rays through the far
    blob alone in a later chunk, rays between them never.  The axes of a Gaussian differ by a factor of up to 2: the
    rotation gradient of a nearly isotropic Gaussian cancels to nothing, which its scale s_g does not see."""
    import math
    cdt = 1.0 / 60 if nr < 128 else 1.0 / 256
    start = int(round(0.2 / cdt))

    def place(m, walls):
        g = torch.Generator().manual_seed(OPAQUE_SEED[nr] if seed is None else seed)
        n = m._mu.shape[0]
        dev = m._mu.device
        r0, L = start * cdt, nr * cdt
        mu, sc = [], []
        for frac, aim in ((0.1, (0.0, 0.5, -0.16)), (0.7, (0.05, 0.5, 0.16))):
            d = torch.tensor(aim)
            d = d / d.norm()
            rr = r0 + frac * L
            s = max(0.15 * rr, 0.075)
            mu.append(rr * d + 0.2 * s * torch.randn(n // 2, 3, generator=g))
            sc.append(math.log(s) + 0.35 * torch.randn(n // 2, 3, generator=g))
        m._mu[:] = torch.cat(mu).float().to(dev)
        m._scaling[:] = torch.cat(sc).float().to(dev)
        m._opacity[:] = (3.0 + 0.5 * torch.randn(n, 1, generator=g)).float().to(dev)
        m._features_dc[:] = (0.4 - 0.5) / R.C0
    return tile_scene(nr, 200, device, "occl", deg=1, seed=9, scale_shift=0.0, opac_shift=0.0, c_deltaT=cdt,
                      edit=place, start=start)


def first_dead_bin(T):
    """[P, rays] from T [P, nr, rays]: the first bin with T < 1e-4, nr where the ray stays live."""
    nr = T.shape[1]
    dead = T < 1e-4
    k = torch.arange(nr)[None, :, None].expand_as(T)
    return torch.where(dead, k, torch.full_like(k, nr)).amin(dim=1)


def window_scene(ng, device=None, mode="occl", scale_shift=1.2, edit=None):
    """Part 4 of test_gpu_tile_edges.py: nr = 40, 6 x 6 rays (one 8 x 8 tile per wall point, partially filled), `ng`
    Gaussians of degree 1 around the stage window (128), the AABB cap (256) and the bin row chunk (1024).  Bins of
    c dT = 1/80 from r = 0.25 to 0.75: the polynomial 1 - exp(-x), so that the faint Gaussians of the larger scenes
    (opacity lowered with ng to keep T above the cut) are not judged by the cancellation of 1 - exp(-x) at x = 1e-5,
    which costs the exp path and the fp32 oracle alike 6e-8 / x."""
    return tile_scene(40, ng, device, mode, nt=6, nphi=6, deg=1, seed=13, scale_shift=scale_shift, opac_shift=0.0,
                      edit=edit, c_deltaT=1.0 / 80, start=20)


def boxes_of(model):
    """[Ng, 6] fp32 3-sigma boxes of a model on the CPU (oracle.torch_ref.bboxes_cuda); the GPU tests pass
    nlosgr.render.bboxes, the engine's own."""
    with torch.no_grad():
        return R.bboxes_cuda(params_of_model(model))


WALK_CLASSES = (96, 56, 28)    # kWalkC0 / C1 / C2 of csrc/nlosgr_tiles.hip: class 0 >= 96 > class 1 >= 56 > ... bins


def walk_scene(device=None, mode="occl", ng=96, seed=5):
    """Part 3 of test_gpu_tile_edges.py: nr = 257 bins of 1.28 / 257 (c dT <= 1/64) from r = 0.16 to 1.44, 96 flat
    slabs facing the wall (standard deviation 0.012 to 0.12 along y, log-uniform: 2.4 to 24 bins, 27 to 270 bins of
    5.7-sigma support along a ray; 0.5 to 1 across, so that every ray passes through both faces of every 3-sigma box,
    far from its edges: the slab test has no near decision), nearly axis-aligned, spread over and beyond the range
    (walks clipped by bin 0 and by the last bin); opacity about 0.27, so that T stays above 1e-2."""
    import math

    def place(m, walls):
        g = torch.Generator().manual_seed(seed)
        n = m._mu.shape[0]
        dev = m._mu.device
        mu = torch.stack([0.3 * (torch.rand(n, generator=g) - 0.5), 0.12 + 1.36 * torch.rand(n, generator=g),
                          0.3 * (torch.rand(n, generator=g) - 0.5)], dim=1)
        sc = torch.stack([_rand_log(g, n, 0.5, 1.0), _rand_log(g, n, 0.012, 0.12), _rand_log(g, n, 0.5, 1.0)], dim=1)
        q = torch.cat([torch.ones(n, 1), 0.1 * torch.randn(n, 3, generator=g)], dim=1)
        m._mu[:] = mu.float().to(dev)
        m._scaling[:] = sc.float().to(dev)
        m._rotation[:] = q.float().to(dev)
        m._opacity[:] = (-1.0 + 0.3 * torch.randn(n, 1, generator=g)).float().to(dev)
        m._features_dc[:] = (0.4 - 0.5) / R.C0
    return tile_scene(257, ng, device, mode, deg=1, seed=seed, scale_shift=0.0, opac_shift=0.0, edit=place)


def walk_lengths(model, geo, cutoff):
    """int [P, Ng, nt, np]: the number of bins of every (Gaussian, ray)'s in-support walk as the tile backward
    counts them (bins ceil(ks - hk) .. floor(ks + hk) clipped to the row; 0: the ray misses the support), in
    float64 from the promoted tables."""
    P = Params64(params_of_model(model))
    tab = tables(geo)
    nr = tab["r"].shape[0]
    r0 = float(tab["r"][0])
    dr = float(tab["r"][-1] - tab["r"][0]) / (nr - 1)
    out = []
    with torch.no_grad():
        s = torch.exp(P._scaling) + 1e-8
        rot = R.quat_to_rotmat_cuda(P._rotation).transpose(1, 2)
        for p in range(tab["wall"].shape[0]):
            d, _ = directions(tab, p)
            u0 = torch.einsum("gab,gb->ga", rot, tab["wall"][p][None, :] - P._mu) / s
            v = torch.einsum("gab,nb->gna", rot, d) / s[:, None, :]
            a = (v * v).sum(-1)
            ts = -(u0[:, None, :] * v).sum(-1) / a
            z = u0[:, None, :] + ts[..., None] * v
            m2 = (z * z).sum(-1)
            hk = torch.sqrt(torch.clamp_min(cutoff * cutoff - m2, 0.0) / a) / dr
            ks = (ts - r0) / dr
            lo = torch.ceil(ks - hk).clamp(0, nr)
            hi = torch.floor(ks + hk).clamp(-1, nr - 1)
            n = torch.where(m2 <= cutoff * cutoff, (hi - lo + 1).clamp_min(0), torch.zeros_like(hi))
            out.append(n.long().view(-1, geo.nt, geo.np))
    return torch.stack(out)


def walk_blocks(L, p, ti, tj, nhalf=64):
    """[(live pairs, sorted classes present)] of every block of wall point p: the backward handles the live (entry,
    ray) pairs of 64 staged entries (here: Gaussians 64 h .. 64 h + 63, which holds while every Gaussian passes the
    tile's cull; Gaussians the cull drops are live on no ray, so the count is a lower bound) and the four rays
    (ti0 + 4 rb + kk, tj0 + rg), kk = 0..3, at a time, and sorts them by class when there are more than 64."""
    ng, nt, nph = L.shape[1], L.shape[2], L.shape[3]
    out = []
    for i0 in range(0, nt, ti):
        for j0 in range(0, nph, tj):
            for rb in range((ti + 3) // 4):
                for rg in range(tj):
                    for h in range(0, ng, nhalf):
                        blk = L[p, h:h + nhalf, i0 + 4 * rb:min(i0 + 4 * rb + 4, i0 + ti, nt), j0 + rg:j0 + rg + 1]
                        if blk.numel():
                            live = blk > 0
                            out.append((int(live.sum()), sorted(set(walk_class(blk[live]).tolist()))))
    return out


def walk_class(length):
    """0..3 as the tile backward ranks a live walk (WALK_CLASSES)."""
    c0, c1, c2 = WALK_CLASSES
    return torch.where(length >= c0, 0, torch.where(length >= c1, 1, torch.where(length >= c2, 2, 3)))


def equivalent_gray(geo, gout, ray_scale):
    """The per-ray upstream that is mathematically the hist upstream gout: gray[p, ij, k] = gout[p, k] att[k]
    hscale[p] sin(theta_i) / ray_scale (float64 from the promoted tables)."""
    tab = tables(geo)
    st = tab["st"][:, :, None].expand(-1, -1, tab["sp"].shape[1]).reshape(tab["st"].shape[0], -1)     # [P, rays]
    return (gout.detach().cpu().double() * tab["att"][None, :] * tab["hscale"][:, None])[:, None, :] * st[:, :, None] \
        / float(ray_scale)


def fp32_oracle(model, geo, mode, c_deltaT, cutoff, selection="support", boxes=None, gout=None, gray=None, ray_scale=1.0):
    """The yardstick: oracle.torch_ref.render_rays_cuda in fp32 (cuda preset; occl, or noocl) over the geometry's own
    tables (origins, directions, r), with aabb_filter's per-ray lists, folded into hist as the kernels do, and torch
    autograd in fp32 of sum(hist gout) + sum(rays gray).  Returns (hist [P, nr], rays [P, rays, nr], the six
    gradients or None, the lists)."""
    cpu = lambda t: t.detach().cpu()
    P = params_of_model(model)
    hist, rays, lists = [], [], []
    for p in range(geo.nwall):
        st, ct, sp, cp = [cpu(t[p]) for t in (geo.sin_theta, geo.cos_theta, geo.sin_phi, geo.cos_phi)]
        d = torch.stack([st[:, None] * cp[None, :], st[:, None] * sp[None, :], ct[:, None].expand(geo.nt, geo.np)],
                        dim=-1).reshape(-1, 3)
        wall = cpu(geo.wall[p])
        o = wall[None, :].expand(d.shape[0], 3).contiguous()
        filt = R.aabb_filter(o, d, cpu(boxes)) if selection == "aabb" else None
        # render_rays_cuda's no-occlusion output carries c dT; the kernels' per-ray output carries ray_scale instead
        rho, _, _ = R.render_rays_cuda(o, d, cpu(geo.r), P, P.features[:, :, 0], wall, P.active_sh_degree, 1.0,
                                       c_deltaT if mode == "occl" else 1.0, 1.0, mode == "occl", filt,
                                       cutoff if cutoff > 0 else None)
        w = st[:, None].expand(geo.nt, geo.np).reshape(-1)
        hist.append(cpu(geo.hscale[p]) * cpu(geo.att) * (rho * w[:, None]).sum(dim=0))
        rays.append(rho * ray_scale)
        lists.append(filt)
    hist, rays = torch.stack(hist), torch.stack(rays)
    grads = None
    if gout is not None or gray is not None:
        loss = 0.0
        if gout is not None:
            loss = loss + (hist * cpu(gout).float()).sum()
        if gray is not None:
            loss = loss + (rays * cpu(gray).float()).sum()
        loss.backward()
        grads = [l.grad if l.grad is not None else torch.zeros_like(l) for l in P.leaves()]
    return hist.detach(), rays.detach(), grads, lists


def rays_absolute(P, geo, mode, c_deltaT, cutoff, selection="support", boxes=None, ray_scale=1.0, subtract=None):
    """[P, rays, nr]: the absolute part of a per-(ray, bin) bound.  Occlusion at c dT > 1/64 forms 1 - exp(-x) by
    subtraction, which loses one fp32 unit roundoff of 1 per selected Gaussian whatever x is: U T_k ray_scale
    sum_g rho_g over the Gaussians of the ray's list with the sample inside their support (W is sum_g rho_g (1 -
    exp(-x_g))).  Otherwise (the polynomial below 1/64, no occlusion) only what fp32 does not resolve: 2^-126.
    subtract: whether the evaluation judged subtracts (None: as the engine does, above 1/64; the fp32 oracle always)."""
    tab = tables(geo)
    P = Params64(P)
    nw, nr, nray = tab["wall"].shape[0], tab["r"].shape[0], tab["st"].shape[1] * tab["sp"].shape[1]
    subtract = c_deltaT > 1.0 / 64 if subtract is None else subtract
    if mode != "occl" or not subtract:
        return torch.full((nw, nray, nr), 2.0 ** -126, dtype=torch.float64)
    sels = _selections(tab, selection, boxes)
    out = []
    with torch.no_grad():
        for p in range(nw):
            x, _ = _points(tab, p)
            pdf = R.gaussian_pdf(x.reshape(-1, 3), P, "cuda", 1.0, _mc(cutoff)).view(-1, nr, nray)
            if sels is not None:
                pdf = pdf * sels[p][:, None, :].double()
            rho = R.albedo(P, tab["wall"][p], "cuda").reshape(-1, 1, 1)
            D = (torch.sigmoid(P._opacity).reshape(-1, 1, 1) * pdf).sum(dim=0)
            T = torch.exp(-c_deltaT * (torch.cumsum(D, dim=0) - D))
            out.append((U * ray_scale * T * ((pdf > 0).double() * rho).sum(dim=0)).t() + 2.0 ** -126)
    return torch.stack(out)


def empty_tile_scene(device=None):
    """Part 6 of test_gpu_tile_edges.py: nr = 40, 9 x 5 rays (tiles of 8 x 8: rows 0..7 and row 8 alone), 12 small
    Gaussians (standard deviation 0.03) in the top of the hidden volume (z about 0.2), which the rays of the last
    theta row (aimed at z = -0.25) miss by more than 5.7 sigma at every wall point: the second tile of every wall
    point has no Gaussian."""
    import math

    def place(m, walls):
        g = torch.Generator().manual_seed(3)
        n = m._mu.shape[0]
        dev = m._mu.device
        mu = torch.tensor([0.0, 0.5, 0.2]) + (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([0.3, 0.3, 0.04])
        m._mu[:] = mu.float().to(dev)
        m._scaling[:] = (math.log(0.03) + 0.1 * torch.randn(n, 3, generator=g)).float().to(dev)
        m._features_dc[:] = (0.4 - 0.5) / R.C0
    return tile_scene(40, 12, device, "occl", deg=1, seed=3, scale_shift=0.0, opac_shift=1.0, edit=place)


def sample_conditioning(P, geo, preset, p, ray, k):
    """What makes the gradient of ONE sample (a one-hot per-ray upstream at wall point p, ray, bin k) hard in fp32,
    per Gaussian and in float64: (|u0|, |z|, kappa) [Ng] each, with u0 = S^-1 R (wall_p - mu) and z = u0 + r_k v the
    sample's whitened position (a small sum of two vectors |u0| long when the sample is near the centre), and
    kappa = (0.5 + sum_i |Y_i(d) f_i|) / rho, the cancellation in the albedo rho = max(0, 0.5 + sum_i Y_i(d) f_i)
    (inf where rho = 0).  Under a dense upstream these average out over the samples and the wall points of a
    Gaussian; under a one-hot upstream the single sample is all there is."""
    P = Params64(P)
    with torch.no_grad():
        tab = tables(geo)
        if preset == "torch":
            s = torch.exp(torch.exp(P._scaling))
            rot = R.build_rotation(torch.nn.functional.normalize(P._rotation))
        else:
            s = torch.exp(P._scaling) + 1e-8
            rot = R.quat_to_rotmat_cuda(P._rotation).transpose(1, 2)
        d = directions(tab, p)[0][ray]
        u0 = torch.einsum("gab,gb->ga", rot, tab["wall"][p][None, :] - P._mu) / s
        z = u0 + tab["r"][k] * torch.einsum("gab,b->ga", rot, d) / s
        f = P.features[:, :, 0]
        K = f.shape[1]
        terms = []
        for i in range(K):           # Y_i(d) f_i: the albedo with every other coefficient zeroed, minus the 0.5
            one = SimpleParams(P, f * torch.nn.functional.one_hot(torch.tensor(i), K).double()[None, :])
            dirn = P._mu - tab["wall"][p][None, :]
            if preset == "torch":
                dn = dirn / dirn.norm(dim=1, keepdim=True)
                terms.append(R.eval_sh(one.deg, one.f.view(-1, 1, K), dn)[:, 0])
            else:
                dn = dirn * (1.0 / (torch.sqrt((dirn * dirn).sum(dim=1, keepdim=True)) + 1e-8))
                terms.append(R.eval_sh_cuda(one.deg, one.f, dn))
        terms = torch.stack(terms, dim=1)
        rho = torch.clamp_min(0.5 + terms.sum(dim=1), 0.0)
        kappa = torch.where(rho > 0, (0.5 + terms.abs().sum(dim=1)) / rho.clamp_min(1e-300),
                            torch.full_like(rho, float("inf")))
        return u0.norm(dim=1), z.norm(dim=1), kappa


class SimpleParams:
    """(features [Ng, K], active degree) for sample_conditioning."""

    def __init__(self, P, f):
        self.f, self.deg = f, int(P.active_sh_degree)
