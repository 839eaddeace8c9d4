"""float64 reference of the batched volume render and its backward, and the per-Gaussian metric the backward
is judged by (plain module, no tests; shared by test_volume_oracle_cpu.py, test_gpu_bwd_edges.py and
test_gpu_fwd_edges.py).

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
