"""float64 reference of the path-C rays API (csrc/nlosgr_rays.hip), its per-Gaussian metric and the scenes of
tests/test_gpu_rays_edges.py and tests/test_rays_oracle_cpu.py (plain module, CPU only, no tests).

The model is the one oracle.torch_ref.render_rays_cuda restates, evaluated on volume_oracle.Params64 leaves.  A ray
sums over the Gaussians of its filter row (an INPUT: int32 [nrays, 257] = count, indices, -1 padding), at the
samples x = o + t_s d:

    D_s = sum_g sigma_g pdf_g(x_s)                                  density
    no occlusion   rho_s = c dT sum_g sigma_g pdf_g rho_g,  T_s = 1
    occlusion      T_s = exp(-c dT sum_{s' < s} D_s'),  W_s = sum_g rho_g (1 - exp(-sigma_g pdf_g c dT)),
                   rho_s = T_s W_s; a sample is live iff T_s >= 1e-4, and a dead sample is 0 in all three outputs

pdf and rho_g are oracle.torch_ref.gaussian_pdf / albedo of the preset ("cuda", or "torch": s = exp(exp(S)), 3DGS
sign convention of the SH basis).  o, d, t, cam and c dT are the fp32 values the kernel reads, promoted, so only
the kernel's arithmetic is measured.  Gradients are torch autograd of sum(g_rho rho + g_dens density + g_tr T) with
the live mask held constant.

The metric.  Every upstream is split into its positive and its negative part (volume_oracle._split_grads); with
G_k [Ng, C] the reference gradient under part k (up to six parts), the gradient is the signed sum of the parts and

    s_g = max_c sum_k |G_k[g, c]|        what the row is made of before the signs cancel
    e_g = max_c |got[g, c] - ref[g, c]|  checked as e_g <= TOL[tensor] s_g for every Gaussian of every tensor

through volume_oracle.gaussian_errors / failures / worst (the bracket is zero: this path culls nothing).  The
forward is judged per ray: max_s |got - ref| <= FWD_TOL max_s |ref| for each of the three outputs.

T >= 1e-4 is a discontinuous decision: Reference.margin is the smallest |T_s / 1e-4 - 1| over every (ray, sample),
dead or alive (inf without occlusion).  Every occlusion scene is built so that it is at least MARGIN = 1e-3 (fp32
moves T by about 1e-5 relative: an exponent below 10 summed in fp32), and then no sample is left out of a comparison.
tune_cdt() places the first dead sample of one ray: c dT is set half way between the optical depths that would kill
sample s* - 1 and sample s*.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from oracle import torch_ref as R

import volume_oracle as VO

CAP = 256             # NLOSGR_MAX_PER_RAY
ROW = CAP + 1
T_DEAD = 1e-4
MARGIN = 1e-3         # the bound volume_oracle.decision_margins' users assert
OUTPUTS = ("rho", "density", "trans")

# The tolerances of tests/test_gpu_rays_edges.py (table in its docstring): 8 x the worst value of fp32_oracle() over
# scenes A, B and D in the metric above, rounded up to one significant digit; tests/test_rays_oracle_cpu.py measures
# it again.  None exceeds what tests/test_gpu_rays.py promises (forward 2e-5, 2e-4 with occlusion; gradients 2e-4,
# 3e-4 with occlusion): rho without occlusion would be 3e-5 and is capped at 2e-5.  T is exactly 1 without occlusion.
TOL = {"mu": 3e-5, "scaling": 3e-5, "rotation": 1e-4, "opacity": 3e-5, "features_dc": 3e-5, "features_rest": 3e-5}
FWD_TOL = {False: {"rho": 2e-5, "density": 9e-6, "trans": 0.0},       # keyed by occlusion
           True: {"rho": 3e-5, "density": 9e-6, "trans": 9e-7}}
assert max(TOL.values()) <= 2e-4 and max(FWD_TOL[False].values()) <= 2e-5 and max(FWD_TOL[True].values()) <= 2e-4


# --------------------------------------------------------------------------------------------
# the model
# --------------------------------------------------------------------------------------------
def row_mask(filt, ng):
    """bool [Ng, nrays]: the Gaussians each filter row names."""
    m = torch.zeros(ng, filt.shape[0], dtype=torch.bool)
    for r in range(filt.shape[0]):
        n = min(max(int(filt[r, 0]), 0), CAP)
        if n:
            m[filt[r, 1:1 + n].long(), r] = True
    return m


def outputs(P, o, d, t, cam, preset, c_deltaT, occl, filt):
    """(rho, density, T, T_raw) [nrays, nsamp] in P's dtype, differentiable in P's leaves; T_raw is the
    transmittance as the exclusive sum continues it (not zeroed on dead samples; ones without occlusion)."""
    dt = P._mu.dtype
    o, d, t, cam = (x.detach().cpu().to(dt) for x in (o, d, t, cam))
    ng, nrays, nsamp = P._mu.shape[0], o.shape[0], t.shape[0]
    x = (o[:, None, :] + d[:, None, :] * t[None, :, None]).reshape(-1, 3)
    pdf = R.gaussian_pdf(x, P, preset).view(ng, nrays, nsamp) * row_mask(filt, ng).to(dt)[:, :, None]
    sig = torch.sigmoid(P._opacity).view(-1, 1, 1)
    rho_g = R.albedo(P, cam, preset).view(-1, 1, 1)
    contrib = pdf * sig
    D = contrib.sum(0)
    if not occl:
        one = torch.ones_like(D.detach())
        return (contrib * rho_g).sum(0) * c_deltaT, D, one, one
    W = (-torch.expm1(-contrib * c_deltaT) * rho_g).sum(0)
    T = torch.exp(-c_deltaT * (torch.cumsum(D, dim=1) - D))
    live = (T.detach() >= T_DEAD).to(dt)
    return T * W * live, D * live, T * live, T.detach()


@dataclass
class Reference:
    rho: torch.Tensor        # [nrays, nsamp] float64
    density: torch.Tensor
    trans: torch.Tensor
    T_raw: torch.Tensor      # not zeroed on dead samples
    dead: torch.Tensor       # bool [nrays, nsamp]
    margin: float            # min |T_s / 1e-4 - 1| (inf without occlusion)
    grads: dict              # name -> [Ng, C]   (volume_oracle.NAMES)
    scale: dict              # name -> [Ng]      s_g
    bracket: dict            # name -> [Ng]      zeros (what volume_oracle.failures / worst expect)
    named: torch.Tensor      # bool [Ng]: some filter row names the Gaussian

    @property
    def fwd(self):
        return (self.rho, self.density, self.trans)

    def first_dead(self):
        """Per ray the index of its first dead sample, -1 for a ray that never dies."""
        return [int(row.int().argmax()) if bool(row.any()) else -1 for row in self.dead]


def _up(u):
    return None if u is None else u.detach().cpu().double()


def reference(P, o, d, t, cam, preset, c_deltaT, occl, filt, ups=(None, None, None)):
    """The float64 forward, the gradient of sum(g_rho rho + g_dens density + g_tr T) for ups = (g_rho, g_dens,
    g_tr) (any may be None), s_g and the decision margin.  P: oracle Params (fp32 or fp64)."""
    P = VO.Params64(P)
    ng = P._mu.shape[0]
    rho, dens, tr, T_raw = outputs(P, o, d, t, cam, preset, c_deltaT, occl, filt)
    leaves = P.leaves()
    shapes = [(ng, int(np.prod(l.shape[1:]))) for l in leaves]
    grads = {n: torch.zeros(s, dtype=torch.float64) for n, s in zip(VO.NAMES, shapes)}
    mass = {n: torch.zeros(s, dtype=torch.float64) for n, s in zip(VO.NAMES, shapes)}
    for out, u in zip((rho, dens, tr), ups):
        u = _up(u)
        if u is None or not out.requires_grad:
            continue
        for s in (1.0, -1.0):
            part = torch.clamp_min(s * u, 0.0)
            if not bool(part.any()):
                continue
            g = torch.autograd.grad(out, leaves, grad_outputs=part, retain_graph=True, allow_unused=True)
            for n, gi, shp in zip(VO.NAMES, g, shapes):
                if gi is not None:
                    grads[n] += s * gi.reshape(shp)
                    mass[n] += gi.reshape(shp).abs()
    dead = T_raw < T_DEAD
    margin = float((T_raw / T_DEAD - 1.0).abs().min()) if occl and T_raw.numel() else float("inf")
    return Reference(rho.detach(), dens.detach(), tr.detach(), T_raw, dead, margin, grads,
                     {n: VO._rowmax(m) for n, m in mass.items()},
                     {n: torch.zeros(ng, dtype=torch.float64) for n in VO.NAMES}, row_mask(filt, ng).any(dim=1))


def fp32_oracle(P, o, d, t, cam, preset, c_deltaT, occl, filt, ups=(None, None, None), literal=False):
    """Another fp32 evaluation of the same sums, with torch autograd: outputs() on fp32 Params.  literal=True (cuda
    preset): oracle.torch_ref.render_rays_cuda itself, which forms alpha as 1 - exp(-x) like the reference's text;
    that difference cancels to 6e-8 absolute, so a ray or a feature row made of small alphas is off by up to 100 %
    in fp32 (the kernel and outputs() use expm1).  The tolerances are taken from the expm1 form, which is never the
    wider of the two.  Returns ((rho, density, T), six gradients in volume_oracle.NAMES order)."""
    P = R.Params(*[l.detach().float() for l in P.leaves()], P.active_sh_degree)
    o, d, t, cam = (x.detach().cpu().float() for x in (o, d, t, cam))
    if literal and preset == "cuda":
        outs = R.render_rays_cuda(o, d, t, P, P.features[:, :, 0], cam, P.active_sh_degree, 1.0, c_deltaT, 1.0, occl,
                                  filt)
    else:
        outs = outputs(P, o, d, t, cam, preset, c_deltaT, occl, filt)[:3]
    loss = sum((out * u.detach().cpu().float()).sum() for out, u in zip(outs, ups) if u is not None and out.requires_grad)
    if torch.is_tensor(loss):
        loss.backward()
    return tuple(x.detach() for x in outs), [l.grad if l.grad is not None else torch.zeros_like(l) for l in P.leaves()]


def forward_worst(got, ref):
    """name -> max over rays of max_s |got - ref| / max_s |ref| for (rho, density, trans); inf for a ray the
    reference leaves at zero and the result does not."""
    out = {}
    for n, a, b in zip(OUTPUTS, got, ref.fwd):
        a = a.detach().cpu().double()
        if b.numel() == 0:
            out[n] = 0.0
            continue
        err, top = (a - b).abs().amax(dim=1), b.abs().amax(dim=1)
        rel = torch.where(top > 0, err / top.clamp_min(1e-300),
                          torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        out[n] = float(rel.max())
    return out


def tune_cdt(P, o, d, t, cam, preset, filt, ray, s_star):
    """c dT (an fp32 value, as a float) that makes sample s_star (>= 1) the first dead sample of `ray`: half way
    between the optical depths that kill s_star - 1 and s_star."""
    with torch.no_grad():
        D = outputs(VO.Params64(P), o[ray:ray + 1], d[ray:ray + 1], t, cam, preset, 1.0, False, filt[ray:ray + 1])[1][0]
    tau = torch.cumsum(D, 0) - D
    mid = 0.5 * float(tau[s_star - 1] + tau[s_star])
    return float(np.float32(math.log(1.0 / T_DEAD) / mid))


# --------------------------------------------------------------------------------------------
# scenes
# --------------------------------------------------------------------------------------------
@dataclass
class Scene:
    P: R.Params            # fp32 leaves on the CPU
    o: torch.Tensor        # [nrays, 3] fp32
    d: torch.Tensor
    t: torch.Tensor        # [nsamp] fp32, increasing
    cam: torch.Tensor      # [3]
    preset: str
    occl: bool
    cdt: float
    filt: torch.Tensor     # int32 [nrays, 257]

    @property
    def deg(self):
        return self.P.active_sh_degree

    @property
    def feats(self):
        """[Ng, K] as the kernel takes them."""
        return self.P.features[:, :, 0].detach().contiguous()

    def args(self):
        return (self.P, self.o, self.d, self.t, self.cam, self.preset, self.cdt, self.occl, self.filt)

    def reference(self, ups=(None, None, None)):
        return reference(*self.args(), ups)

    def fp32(self, ups=(None, None, None), literal=False):
        return fp32_oracle(*self.args(), ups, literal)

    def upstreams(self, seed=5):
        g = torch.Generator().manual_seed(seed)
        return tuple(torch.randn(self.o.shape[0], self.t.shape[0], generator=g) for _ in range(3))


# SH degrees 0 to 3 spread over the (preset, occlusion) cases
DEG = {("cuda", False): 0, ("cuda", True): 3, ("torch", False): 2, ("torch", True): 1}
CDT_FREE = 0.02       # c dT without occlusion (the kernel only scales rho by it)
CAM = (0.05, 0.0, -0.02)


def params(ng, deg, preset, seed, scale_shift=0.5, opac_shift=1.0, k_deg=None):
    """nlosgr.GaussianParams.synthetic on the CPU as fp32 oracle Params: log-scales + scale_shift under the cuda
    preset (the torch preset's double exponential makes every standard deviation >= 1 already), opacity +
    opac_shift.  k_deg: allocate the features of SH degree k_deg >= deg ((k_deg + 1)^2 columns) and evaluate
    degree deg."""
    from nlosgr.model import GaussianParams
    m = GaussianParams.synthetic(ng, deg if k_deg is None else k_deg, preset=preset, device="cpu", seed=seed)
    with torch.no_grad():
        if preset == "cuda":
            m._scaling.add_(scale_shift)
        m._opacity.add_(opac_shift)
    return R.Params(*[x.detach() for x in (m._mu, m._scaling, m._rotation, m._opacity, m._features_dc,
                                            m._features_rest)], deg)


def rays(nrays, seed):
    """The rays of tests/test_gpu_rays.py::_scene: origins on the wall y = 0, directions into the volume."""
    g = torch.Generator().manual_seed(seed + 1)
    o = torch.zeros(nrays, 3)
    o[:, 0] = torch.rand(nrays, generator=g) - 0.5
    o[:, 2] = torch.rand(nrays, generator=g) - 0.5
    th = 0.3 + 1.0 * torch.rand(nrays, generator=g)
    ph = 0.8 + 1.5 * torch.rand(nrays, generator=g)
    d = torch.stack([torch.sin(th) * torch.cos(ph), torch.sin(th) * torch.sin(ph), torch.cos(th)], 1)
    return o.contiguous(), d.contiguous()


def t_grid(nsamp, uniform=False):
    """nsamp increasing sample distances from 0.1 to 1.4, non-uniform (steps growing by 1.9 over the ray)."""
    u = torch.linspace(0.0, 1.0, nsamp, dtype=torch.float64) if nsamp > 1 else torch.zeros(1, dtype=torch.float64)
    return (0.1 + 1.3 * (u if uniform else 0.7 * u + 0.3 * u * u)).float().contiguous()


def rows(lists):
    """int32 [nrays, 257] filter rows from one index list per ray."""
    f = torch.full((len(lists), ROW), -1, dtype=torch.int32)
    for r, idx in enumerate(lists):
        idx = list(idx)
        assert len(idx) <= CAP
        f[r, 0] = len(idx)
        if idx:
            f[r, 1:1 + len(idx)] = torch.tensor(idx, dtype=torch.int32)
    return f


def drop_rows(nrays, ng):
    """Ray r names every Gaussian but r % ng (index order), so the rows differ from ray to ray."""
    return rows([[g for g in range(ng) if ng == 1 or g != r % ng] for r in range(nrays)])


def _finish(P, o, d, t, preset, occl, filt, tune, cdt_occl=0.3):
    cam = torch.tensor(CAM)
    if not occl:
        cdt = float(np.float32(CDT_FREE))
    elif tune is None:
        cdt = float(np.float32(cdt_occl))
    else:
        cdt = tune_cdt(P, o, d, t, cam, preset, filt, *tune)
    return Scene(P, o, d, t, cam, preset, occl, cdt, filt)


# A. sample counts: where ray 0 first dies under occlusion (None: it does not)
A_NSAMP = (1, 63, 64, 65, 129, 200)
A_FIRST_DEAD = {1: None, 63: 62, 64: 63, 65: 64, 129: 128, 200: 150}
A_SEED = {"cuda": 34, "torch": 20}   # chosen so that every occlusion case keeps MARGIN (the CPU tests assert it)


def scene_A(nsamp, preset, occl):
    """12 Gaussians, 5 rays, a non-uniform t.  Rays 0-3 name all Gaussians but one, ray 4 names one Gaussian only
    and never dies.  Under occlusion c dT puts ray 0's first dead sample at A_FIRST_DEAD[nsamp]: lane 63 of chunk
    0 (nsamp 64), lane 0 of chunk 1 (65), lane 0 of chunk 2 (129), inside chunk 2 (200), the last sample (63)."""
    seed = A_SEED[preset]
    P = params(12, DEG[(preset, occl)], preset, seed)
    o, d = rays(5, seed)
    filt = drop_rows(5, 12)
    filt[4] = rows([[7]])[0]
    s = A_FIRST_DEAD[nsamp]
    return _finish(P, o, d, t_grid(nsamp), preset, occl, filt, None if s is None else (0, s))


# B. selected counts per ray
B_COUNTS = ((0, 1, 64), (65, 256, 1), (256,), (0,), (65,))
B_NG, B_NSAMP = 300, 70
B_SEED = {"cuda": 49, "torch": 49}


def scene_B(counts, preset, occl):
    """300 Gaussians, one ray per entry of `counts`, whose row holds that many Gaussians (a random subset in index
    order), 70 samples.  Under occlusion the ray with the longest row (of 64 and more) first dies at sample 40."""
    seed = B_SEED[preset]
    P = params(B_NG, DEG[(preset, occl)], preset, seed)
    o, d = rays(len(counts), seed)
    g = torch.Generator().manual_seed(seed + 7)
    filt = rows([sorted(torch.randperm(B_NG, generator=g)[:n].tolist()) for n in counts])
    big = max(range(len(counts)), key=lambda r: counts[r])
    return _finish(P, o, d, t_grid(B_NSAMP), preset, occl, filt, (big, 40) if counts[big] >= 64 else None)


# C. more than one ray per backward slot
C_NRAYS, C_NG, C_NSAMP, C_SLOTS = 1030, 7, 65, 1024
C_SEED = {"cuda": 51, "torch": 28}


def scene_C(preset, occl):
    """1030 rays (slots 0 to 5 of the 1024 take two rays each), 7 Gaussians, 65 samples.  Rays 0-2 have an empty
    row and rays 1024-1026 do not; rays 3-5 have a row and rays 1027-1029 are empty.  The rays repeat 10 distinct
    (origin, direction) pairs (ray r has geometry r % 10; rays r and r + 1024 differ), so that the occlusion
    threshold has 10 margins to keep, not 1030.  Under occlusion ray 1024 first dies at sample 40."""
    seed = C_SEED[preset]
    P = params(C_NG, DEG[(preset, occl)], preset, seed)
    o10, d10 = rays(10, seed)
    idx = torch.arange(C_NRAYS) % 10
    filt = drop_rows(C_NRAYS, C_NG)
    for r in (0, 1, 2, 1027, 1028, 1029):
        filt[r] = rows([[]])[0]
    return _finish(P, o10[idx].contiguous(), d10[idx].contiguous(), t_grid(C_NSAMP), preset, occl, filt, (1024, 40))


# D. upstreams
D_NSAMP = 130
D_SEED = {"cuda": 34, "torch": 47}


def scene_D(preset, occl, k16=False):
    """12 Gaussians, 5 rays, 130 samples; under occlusion ray 0 first dies at sample 100 (so samples 0, 63 and 64
    are live on it and sample 129 is dead).  k16: 16 feature columns evaluated at SH degree 1."""
    seed = D_SEED[preset]
    P = params(12, 1 if k16 else DEG[(preset, occl)], preset, seed, k_deg=3 if k16 else None)
    o, d = rays(5, seed)
    return _finish(P, o, d, t_grid(D_NSAMP), preset, occl, drop_rows(5, 12), (0, 100))


def one_hot(scene, s):
    """Upstreams that are zero but at sample s of every ray (1, -0.7 and 1.3 for rho, density and T)."""
    ups = []
    for v in (1.0, -0.7, 1.3):
        u = torch.zeros(scene.o.shape[0], scene.t.shape[0])
        u[:, s] = v
        ups.append(u)
    return tuple(ups)


# E. the largest admitted nsamp
E_NSAMP = 8192


def scene_E(preset, occl):
    """8192 samples (uniform t), 2 rays, 3 broad Gaussians (cuda preset: log-scales + 1.5), the third one dim
    (opacity - 3).  Ray 0 names all three and under occlusion first dies at sample 2000 (chunk 31; a step changes T
    by 0.5 %, so the margin holds); ray 1 names the dim one only and never dies."""
    P = params(3, DEG[(preset, occl)], preset, 61, scale_shift=1.5)
    with torch.no_grad():
        P._opacity[2] -= 3.0
    o, d = rays(2, 61)
    filt = rows([[0, 1, 2], [2]])
    return _finish(P, o, d, t_grid(E_NSAMP, uniform=True), preset, occl, filt, (0, 2000))


# F. the filter
def boxes(ng, seed, half=(0.1, 0.4)):
    """[Ng, 6] fp32 boxes (min xyz, max xyz) with centres in the hidden volume and half-widths in `half`."""
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor([0.0, 0.5, 0.0]) + (torch.rand(ng, 3, generator=g) - 0.5) * 0.8
    h = half[0] + (half[1] - half[0]) * torch.rand(ng, 3, generator=g)
    return torch.cat([c - h, c + h], dim=1).float().contiguous()


F_NG, F_NRAYS = (0, 1, 63, 64, 65, 129), (1, 3, 5)


def filter_case(ng, nrays):
    """(o, d, boxes) of the filter's size sweep: fewer boxes than a 64-lane block, one more than a block, none;
    fewer rays than a workgroup's four and one more.  Between a twentieth and a half of the (ray, box) pairs hit
    (a single box is made large enough for some ray to hit it)."""
    o, d = rays(nrays, 70 + ng)
    return o, d, boxes(ng, 80 + ng, (0.45, 0.5) if ng == 1 else (0.1, 0.4))


def slab_margin(o, d, bb):
    """The smallest |tmax - tmin| and |tmax| over every (ray, box), in float64: how far the fp32 slab test stays
    from a tie (which the kernel and the oracle, both fp32 with the same operations, would still decide alike)."""
    inv = 1.0 / (d.double() + 1e-8)
    t0 = (bb.double()[None, :, 0:3] - o.double()[:, None, :]) * inv[:, None, :]
    t1 = (bb.double()[None, :, 3:6] - o.double()[:, None, :]) * inv[:, None, :]
    tmin, tmax = torch.minimum(t0, t1).amax(-1), torch.maximum(t0, t1).amin(-1)
    return float(torch.minimum((tmax - tmin).abs(), tmax.abs()).min()) if bb.shape[0] else float("inf")


def cap_midblock_boxes():
    """(o, d, boxes) of the 256-cap inside a 64-Gaussian block: 400 boxes strung along one ray, every third
    (and boxes 1 to 8) moved out of the ray's way, so that the 256th hit falls inside a block with more hits behind it
    in the same block; a second ray misses everything, a third one hits all but the moved ones from the other
    end."""
    ng = 400
    c = torch.zeros(ng, 3)
    c[:, 1] = 0.2 + 0.002 * torch.arange(ng)
    moved = (torch.arange(ng) % 3 == 0) | ((torch.arange(ng) >= 1) & (torch.arange(ng) <= 8))
    c[moved, 0] += 5.0
    h = torch.full((ng, 3), 0.05)
    bb = torch.cat([c - h, c + h], dim=1).float().contiguous()
    o = torch.tensor([[0.01, 0.0, 0.02], [0.0, 0.0, 0.0], [0.02, 2.0, -0.01]])
    d = torch.tensor([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.001, -1.0, 0.002]])
    return o.contiguous(), d.contiguous(), bb, moved


def special_rays():
    """(o, d, boxes, the hits each ray must select): directions with a component exactly 0 (the slab test divides
    by 0 + 1e-8) and negative components, an origin inside a box, a box wholly behind the origin, a ray that hits
    nothing."""
    bb = torch.tensor([[-0.1, 0.3, -0.1, 0.1, 0.5, 0.1],      # 0: ahead of the rays along +y
                       [-0.1, -0.6, -0.1, 0.1, -0.4, 0.1],    # 1: behind the wall
                       [0.25, 0.05, 0.25, 0.45, 0.25, 0.45],  # 2: holds the origin of ray 3
                       [-0.5, 0.6, -0.5, -0.3, 0.8, -0.3]])   # 3: off to one side
    o = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.35, 0.15, 0.35], [0.0, 0.0, 0.0],
                      [0.0, 0.0, 0.0]])
    d = torch.tensor([[0.0, 1.0, 0.0],           # two components exactly 0: box 0, not box 1 behind it
                      [0.0, 0.96, 0.28],         # one component exactly 0: box 0
                      [0.0, -1.0, 0.0],          # a negative axis direction from beyond: boxes 0 and 1
                      [-0.6, 0.0, -0.8],         # from inside box 2, negative components and a zero
                      [-0.4 / 0.9, 0.7 / 0.9, -0.4 / 0.9],   # negative components: box 3
                      [1.0, 0.0, 0.0]])          # along the wall: nothing
    return o.contiguous(), d.contiguous(), bb.contiguous(), [[0], [0], [0, 1], [2], [3], []]
