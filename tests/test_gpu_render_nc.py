"""The non-confocal Gaussian renderer (nlosgr_render_nc_fwd / _bwd, nlosgr.render_nc) on the GPU against the float64
oracle tests/render_nc_oracle.py, with volume_oracle's metrics: the forward per row, |got - ref| <= TOL_F rowmax +
the row's bracket max_k |dense - culled|; the backward per Gaussian and tensor, e_g <= TOL_G s_g + b_g under a seeded
normal upstream.  No sample is left out of a comparison: at cutoff 3, where a sample at the support's edge is worth
1e-2 of the peak, the forward is bracketed per bin by the references at 3 x 0.999 and 3 x 1.001 (every term is
non-negative, so the row is monotone in the support).

Base scenes: volume_oracle.compact_scene("cuda") and parity_scene("torch", "noocl", 97) (48 Gaussians, a 2 x 3 wall,
6 x 6 rays, 97 bins) with the lasers displaced from the sensed points by up to +-0.3 in x and z (seeded; max b/2 is
asserted below r0, so every bin holds a path there).

Tolerances: 4 x the worst value measured on the MI355X over every case of this file (pytest -s prints the table),
rounded up to one digit, capped by what the project promises for the confocal renderer (test_gpu_parity.FWD_RTOL =
2e-5, GRAD_RTOL = 2e-4):

                     forward  mu       scaling  rotation opacity  features_dc features_rest
    measured worst   7.03e-7  5.14e-6  6.18e-6  8.44e-6  7.84e-6  1.37e-6     1.23e-6
    4 x, one digit   3e-6     3e-5     3e-5     4e-5     4e-5     6e-6        5e-6

The forward's worst is the cuda base scene at 5.7 sigma, the backward's the training step (its upstream is formed
from the fp32 render, the reference's from the float64 one); without it the backward's worst values are 1.2e-6,
5.1e-6, 4.9e-6, 3.1e-6, 1.7e-7, 2.5e-7.  The backward of the 1030-Gaussian case is judged at the cap and is not part
of these maxima (test_gaussian_counts says why).  The per-case table is in DESIGN.md section 7.
"""
import pytest
import torch

from conftest import ROOT  # noqa: F401

import render_nc_oracle as NCO
import volume_oracle as VO

pytestmark = pytest.mark.gpu

TOL_F = 3e-6
TOL_G = {"mu": 3e-5, "scaling": 3e-5, "rotation": 4e-5, "opacity": 4e-5, "features_dc": 6e-6, "features_rest": 5e-6}
assert TOL_F <= 2e-5 and max(TOL_G.values()) <= 2e-4

_TABLE = {}


@pytest.fixture(scope="module", autouse=True)
def _print_table():
    yield
    cols = ["forward"] + list(VO.NAMES)
    print("\n\nworst measured value per case (forward per row; backward per Gaussian)\n" + f"{'case':<34}"
          + "".join(f"{c:>15}" for c in cols))
    for case, row in _TABLE.items():
        print(f"{case:<34}" + "".join(f"{row.get(c, 0.0):>15.2e}" for c in cols))
    rows = [r for case, r in _TABLE.items() if not case.endswith("(cap)")]
    if rows:
        print(f"{'all but (cap)':<34}" + "".join(f"{max(r.get(c, 0.0) for r in rows):>15.2e}" for c in cols))


def _dev():
    return torch.device("cuda:0")


def _args(model):
    from nlosgr import features_flat
    return [model._mu.detach(), model._scaling.detach(), model._rotation.detach(), model._opacity.detach(),
            features_flat(model).detach().contiguous()]


def _cfg(preset, cutoff, deg):
    from nlosgr.render import RenderConfig
    return RenderConfig(preset=preset, mode="noocl", sh_degree=deg, cutoff=cutoff)


def _displaced(geo, amp=0.3, seed=15):
    g = torch.Generator().manual_seed(seed)
    d = (torch.rand(geo.nwall, 3, generator=g) * 2 - 1) * amp
    d[:, 1] = 0.0
    lasers = (geo.wall.cpu() + d).float().to(geo.wall.device).contiguous()
    halfb = 0.5 * (lasers - geo.wall).double().norm(dim=1).max()
    assert float(halfb) < float(geo.r[0]), "a bin of the scene holds no path: choose a smaller displacement"
    return lasers


def _gout(geo, seed=5):
    return torch.randn(geo.nwall, geo.nr, generator=torch.Generator().manual_seed(seed))


def _run(model, geo, lasers, cfg, gout=None):
    from nlosgr.render_nc import render_nc_backward, render_nc_forward
    a = _args(model)
    h = render_nc_forward(*a, geo, lasers, cfg)
    if gout is None:
        return h
    return h, render_nc_backward(*a, geo, lasers, cfg, gout.to(h.device).float().contiguous())


def _judge(case, model, geo, lasers, preset, cutoff, gout=None, need_rows=True, ref=None, tol=None):
    """Forward and backward against the float64 reference; prints and records the worst values, then asserts."""
    gout = _gout(geo) if gout is None else gout
    deg = int(model.active_sh_degree)
    ref = NCO.reference(VO.params_of_model(model), geo, lasers, preset, cutoff, gout) if ref is None else ref
    h, got = _run(model, geo, lasers, _cfg(preset, cutoff, deg), gout)
    fwd = VO.forward_worst(h, ref)
    named = VO.as_named(got)
    worst = VO.worst(named, ref)
    print(f"\n{case}: forward {fwd:.2e}; " + ", ".join(f"{n} {v:.2e}" for n, v in worst.items()))
    row = _TABLE.setdefault(case, {})
    for n, v in list(worst.items()) + [("forward", fwd)]:
        row[n] = max(row.get(n, 0.0), v)
    bad = VO.failures(named, ref, TOL_G if tol is None else tol)
    assert fwd <= TOL_F, f"forward {fwd:.3e} of a row's maximum, tolerance {TOL_F:.1e}"
    assert not bad, f"{len(bad)} (tensor, Gaussian, e_g, s_g, b_g) beyond tolerance, first: {bad[:6]}"
    if need_rows:
        for n, s in ref.scale.items():
            assert s.numel() == 0 or float(s.max()) > 0, f"{n}: no non-zero reference row"
    K = (deg + 1) ** 2
    assert bool((got[4][:, K:] == 0).all())
    return h, got, ref


# ---------------------------------------------------------------------------------------------------------
# base scenes
# ---------------------------------------------------------------------------------------------------------
_BASE = {}


def _base(preset):
    if preset not in _BASE:
        model, geo, _ = (VO.compact_scene("cuda", device=_dev()) if preset == "cuda"
                         else VO.parity_scene("torch", "noocl", 97, _dev()))
        _BASE[preset] = dict(model=model, geo=geo, lasers=_displaced(geo), gout=_gout(geo), ref={})
    return _BASE[preset]


def _base_ref(preset, cutoff):
    b = _base(preset)
    if cutoff not in b["ref"]:
        b["ref"][cutoff] = NCO.reference(VO.params_of_model(b["model"]), b["geo"], b["lasers"], preset, cutoff, b["gout"])
    return b["ref"][cutoff]


@pytest.mark.parametrize("cutoff", [0.0, 5.7])
@pytest.mark.parametrize("preset", ["cuda", "torch"])
def test_forward_and_backward_against_float64(preset, cutoff):
    """Dense and at 5.7 sigma: every row and every Gaussian of all six tensors."""
    b = _base(preset)
    _, _, ref = _judge(f"base {preset} cutoff {cutoff}", b["model"], b["geo"], b["lasers"], preset, cutoff, b["gout"],
                       ref=_base_ref(preset, cutoff))
    assert float((ref.hist - NCO.forward(VO.params_of_model(b["model"]), b["geo"], b["geo"].wall, preset,
                                         cutoff)).abs().max()) > 1e-2 * float(ref.hist.max())   # not the confocal rows


@pytest.mark.parametrize("preset", ["cuda", "torch"])
def test_forward_at_cutoff_3_is_bracketed_per_bin(preset):
    """ref(3 x 0.999) - TOL_F rowmax <= got <= ref(3 x 1.001) + TOL_F rowmax in every bin (measured width of the
    bracket on the cuda scene: 2.0e-3 of the row's maximum; a dropped or doubled ray or a shifted bin is 1e-2 and up,
    the fp32 error of m^2 1.4e-5 relative)."""
    b = _base(preset)
    P = VO.params_of_model(b["model"])
    lo = NCO.forward(P, b["geo"], b["lasers"], preset, 3.0 * 0.999)
    hi = NCO.forward(P, b["geo"], b["lasers"], preset, 3.0 * 1.001)
    top = hi.amax(dim=1, keepdim=True)
    got = _run(b["model"], b["geo"], b["lasers"], _cfg(preset, 3.0, 3)).cpu().double()
    width = float(((hi - lo) / top).max())
    under, over = float(((lo - got) / top).max()), float(((got - hi) / top).max())
    print(f"\n{preset} cutoff 3: bracket width {width:.2e} of rowmax; below by {under:.2e}, above by {over:.2e}")
    _TABLE[f"bracket {preset} cutoff 3"] = {"forward": max(under, over, 0.0)}
    assert float(top.min()) > 0 and bool((hi >= lo).all())
    assert under <= TOL_F and over <= TOL_F


def test_backward_support_is_the_forward_support_at_cutoff_3():
    """SH degree 0: d_opacity[g] = (1 - sigma_g) sum_pk G hist_g with hist_g the forward of Gaussian g alone, so a
    sample the backward takes and the forward drops (or the reverse) shows at 1e-2 of a Gaussian's peak."""
    b = _base("cuda")
    geo, lasers = b["geo"], b["lasers"]
    a = [t[:16].contiguous() for t in _args(b["model"])]
    cfg = _cfg("cuda", 3.0, 0)
    from nlosgr.render_nc import render_nc_backward, render_nc_forward
    G = b["gout"].to(_dev()).float().contiguous()
    d_o = render_nc_backward(*a, geo, lasers, cfg, G)[3].cpu().double()
    sig = torch.sigmoid(a[3].reshape(-1).cpu().double())
    worst = 0.0
    for g in range(16):
        hg = render_nc_forward(*[t[g:g + 1].contiguous() for t in a], geo, lasers, cfg).cpu().double()
        terms = G.cpu().double() * hg
        want, scale = (1.0 - sig[g]) * terms.sum(), (1.0 - sig[g]) * terms.abs().sum()
        assert float(scale) > 0
        worst = max(worst, float((d_o[g] - want).abs() / scale))
    print(f"\nbackward support = forward support: worst |d_opacity - (1 - sigma) sum G hist_g| / sum |G hist_g| {worst:.2e}")
    assert worst <= TOL_G["opacity"]


# ---------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------
def _scene(preset="cuda", T=97, ng=8, ns=4, wall=(1, 2), deg=3, edit=None, seed=3, scale_shift=0.0):
    """parity_scene with a window of 0.6 from r0 about 0.3 whatever T is, lasers displaced by up to 0.15."""
    deltaT = 0.6 / T
    start = max(1, T // 2)
    model, geo, _ = VO.parity_scene(preset, "noocl", T, _dev(), scale_shift=scale_shift, ng=ng, ns=ns, wall=wall, seed=seed,
                                    edit=edit, start=start, deltaT=deltaT)
    if deg == 4:
        from nlosgr import GaussianParams
        model = GaussianParams.synthetic(ng, 4, preset=preset, device=_dev(), seed=seed)
    model.active_sh_degree = deg
    return model, geo, _displaced(geo, 0.15)


@pytest.mark.parametrize("nr", [1, 17, 97, 1030])
def test_row_lengths(nr):
    """1030 bins cross the forward's 1024 bins per pass; 1 and 17 leave most of a wave without a bin."""
    model, geo, lasers = _scene(T=nr)
    assert geo.nr == nr
    _judge(f"nr={nr}", model, geo, lasers, "cuda", 5.7)


GRAD_CAP = 2e-4    # test_gpu_parity.GRAD_RTOL: what the project promises for the confocal backward


@pytest.mark.parametrize("ng", [1, 65, 151, 1030])
def test_gaussian_counts(ng):
    """One Gaussian; one more than a wave of the forward's cull; 151: a last backward workgroup of three waves;
    1030: a second chunk of the forward's cull (1024 Gaussians per chunk), at 17 bins, standard deviation as the
    65's (log-scale + 0.9).  The forward of the 1030 is judged at TOL_F like every other; their backward at GRAD_CAP,
    not at TOL_G: among a thousand Gaussians a few are seen by a handful of samples in their 5-sigma tail only, where
    the fp32 position error m_c |u0| U of test_gpu_bwd_edges.py is the whole relative error of the row (measured:
    scaling 6.3e-5 and rotation 8.6e-5 of s_g for two such Gaussians with s_g 1e-5 .. 1e-6 of the scene's largest;
    every other Gaussian within TOL_G).  The backward has no path of its own at this count (one wave per Gaussian)."""
    model, geo, lasers = _scene(ng=ng, T=33 if ng < 1000 else 17, scale_shift=0.0 if ng < 1000 else 0.9)
    if ng < 1000:
        _judge(f"ng={ng}", model, geo, lasers, "cuda", 5.7)
    else:
        _judge(f"ng={ng} (cap)", model, geo, lasers, "cuda", 5.7, tol=GRAD_CAP)


def test_no_gaussians():
    from nlosgr.render_nc import render_nc_backward, render_nc_forward
    model, geo, lasers = _scene()
    a = [t[:0].contiguous() for t in _args(model)]
    cfg = _cfg("cuda", 5.7, 3)
    h = torch.full((geo.nwall, geo.nr), 7.0, device=_dev())
    h.copy_(render_nc_forward(*a, geo, lasers, cfg))
    assert bool((h == 0).all())
    got = render_nc_backward(*a, geo, lasers, cfg, _gout(geo).to(_dev()))
    assert [tuple(t.shape) for t in got] == [(0, 3), (0, 3), (0, 4), (0,), (0, 16)]


def test_one_measurement_and_one_laser_for_many():
    model, geo, lasers = _scene(wall=(1, 1))
    assert geo.nwall == 1
    _judge("nmeas=1", model, geo, lasers, "cuda", 5.7)
    model, geo, lasers = _scene(wall=(2, 2))
    _judge("nlaser=1", model, geo, lasers[2:3].contiguous(), "cuda", 5.7)


def test_bins_no_path_reaches_are_exactly_zero():
    """One measurement's laser at b = 2 (r0 + 10.5 dr): its bins 0..10 hold no path and are exactly zero, bins 11..
    and the other measurement are in parity, and so are the gradients (the upstream of the empty bins is finite
    here and must not reach anything; a NaN there must not either)."""
    from nlosgr.render_nc import render_nc_backward
    model, geo, lasers = _scene(T=97)
    r0, dr = float(geo.r[0]), float(geo.r[1] - geo.r[0])
    lasers = lasers.clone()
    lasers[0] = geo.wall[0] + torch.tensor([0.0, 0.0, 2.0 * (r0 + 10.5 * dr)], device=_dev())
    for cutoff in (0.0, 5.7):
        h, got, ref = _judge(f"no-path bins cutoff {cutoff}", model, geo, lasers, "cuda", cutoff)
        assert bool((ref.hist[0, :11] == 0).all()) and bool((ref.hist[0, 11:] > 0).all())
        assert bool((h[0, :11] == 0).all()) and bool((h[0, 11:] > 0).all())
        gout = _gout(geo)
        poisoned = gout.clone()
        poisoned[0, :11] = float("nan")
        again = render_nc_backward(*_args(model), geo, lasers, _cfg("cuda", cutoff, 3), poisoned.to(_dev()))
        assert all(torch.equal(x, y) for x, y in zip(got, again))


def _edge_edit(m, walls):
    """Gaussians 0..5 by hand (standard deviations 0.05 x (1, 1.3, 0.8): an isotropic Gaussian's rotation gradient is
    zero, and its float64 reference rounding noise): wholly outside the angular grid, wholly beyond the window,
    cut by the grid's edge, cut by the first bin, cut by the last bin, and a clamped albedo."""
    dev = m._mu.device
    m._scaling[:6] = torch.log(0.05 * torch.tensor([1.0, 1.3, 0.8], device=dev))
    m._mu[0] = torch.tensor([3.0, 0.5, 0.0], device=dev)
    m._mu[1] = torch.tensor([0.0, 2.5, 0.0], device=dev)
    m._mu[2] = torch.tensor([0.26, 0.26, 0.26], device=dev)
    m._mu[3] = torch.tensor([0.25, 0.3, 0.25], device=dev)
    m._mu[4] = torch.tensor([0.0, 0.9, 0.05], device=dev)
    m._features_dc[:5] = (0.4 - 0.5) / VO.R.C0        # albedo 0.4 for the placed ones,
    m._features_rest[:5] = 0.0
    m._features_dc[5] = -3.0                            # 0.5 + SH = 0.5 - 3 C0 < 0 from every sensed point
    m._features_rest[5] = 0.0


def _reached(P, geo, lasers, preset, cutoff):
    """bool [nmeas, Ng]: measurement p has a sample inside Gaussian g's support (float64, the renderer's points)."""
    tab = VO.tables(geo)
    L = NCO.lasers64(lasers, geo.nwall)
    out = []
    with torch.no_grad():
        for p in range(geo.nwall):
            x, _, q = NCO.points_nc(tab, p, L[p])
            pdf = VO.R.gaussian_pdf(x.reshape(-1, 3), P, preset, 1.0, cutoff)
            out.append(((pdf > 0) & (q.reshape(1, -1) > 0)).any(dim=1))
    return torch.stack(out)


@pytest.mark.parametrize("cutoff", [3.0, 5.7])
def test_gaussians_at_the_edges_of_the_grid_and_the_window(cutoff):
    """At 5.7 sigma forward and gradients are in parity; at 3 sigma the forward is bracketed per bin (the edge
    samples are worth 1e-2 of a peak there).  At both, the Gaussians no sample reaches get exactly zero rows and the
    clamped albedo stops the feature, opacity and mu-through-SH gradients."""
    model, geo, lasers = _scene(ng=12, ns=6, wall=(2, 2), edit=_edge_edit)
    Pm = VO.params_of_model(model)
    P = VO.Params64(Pm)
    reach = _reached(P, geo, lasers, "cuda", 5.7 * 1.001)
    assert not bool(reach[:, 0].any()) and not bool(reach[:, 1].any())
    assert bool(_reached(P, geo, lasers, "cuda", 3.0 * 0.999)[:, 2:5].any(dim=0).all())   # the cut ones are reached
    assert float(VO.R.albedo(P, VO.tables(geo)["wall"][0], "cuda")[5].detach()) == 0.0
    gout = _gout(geo)
    if cutoff == 3.0:
        lo = NCO.forward(Pm, geo, lasers, "cuda", 3.0 * 0.999)
        hi = NCO.forward(Pm, geo, lasers, "cuda", 3.0 * 1.001)
        top = hi.amax(dim=1, keepdim=True)
        h, grads = _run(model, geo, lasers, _cfg("cuda", 3.0, 3), gout)
        got = h.cpu().double()
        under, over = float(((lo - got) / top).max()), float(((got - hi) / top).max())
        print(f"\nedges cutoff 3: below the bracket by {under:.2e}, above by {over:.2e} of rowmax")
        _TABLE["edges cutoff 3 (bracket)"] = {"forward": max(under, over, 0.0)}
        assert under <= TOL_F and over <= TOL_F
    else:
        h, grads, ref = _judge(f"edges cutoff {cutoff}", model, geo, lasers, "cuda", cutoff, gout)
        assert all(float(ref.scale["mu"][g]) > 0 for g in (2, 3, 4))
    for t in grads:
        assert bool((t[0] == 0).all()) and bool((t[1] == 0).all())              # outside: exactly zero rows
    assert bool((grads[4][5] == 0).all())                                        # the clamp stops dL/dfeatures
    assert float(grads[3][5]) == 0.0                                             # and rho = 0 leaves nothing for sigma


@pytest.mark.parametrize("preset,deg", [("cuda", 0), ("cuda", 3), ("torch", 0), ("torch", 4)])
def test_sh_degrees(preset, deg):
    model, geo, lasers = _scene(preset=preset, ng=12, T=33, deg=deg)
    assert _args(model)[4].shape[1] == (25 if deg == 4 else 16)
    _judge(f"{preset} degree {deg}", model, geo, lasers, preset, 5.7, need_rows=deg > 0)


# ---------------------------------------------------------------------------------------------------------
# determinism
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", [0.0, 3.0])
def test_runs_subsets_permutations_and_one_laser_are_bitwise(cutoff):
    from nlosgr.render_nc import render_nc_backward, render_nc_forward
    b = _base("cuda")
    model, geo, lasers = b["model"], b["geo"], b["lasers"]
    cfg = _cfg("cuda", cutoff, 3)
    a = _args(model)
    G = b["gout"].to(_dev()).float().contiguous()
    h1, g1 = _run(model, geo, lasers, cfg, G)
    h2, g2 = _run(model, geo, lasers, cfg, G)
    assert torch.equal(h1, h2) and all(torch.equal(x, y) for x, y in zip(g1, g2))
    # measurements [2:5] alone give those rows
    sub = render_nc_forward(*a, geo.slice(2, 5), lasers[2:5].contiguous(), cfg)
    assert torch.equal(sub, h1[2:5])
    idx = torch.tensor([4, 0, 3])
    assert torch.equal(render_nc_forward(*a, geo.rows(idx), lasers[idx.to(_dev())].contiguous(), cfg), h1[idx.to(_dev())])
    # a permutation of the Gaussians permutes the backward's rows (and appending Gaussians leaves them)
    perm = torch.randperm(a[0].shape[0], generator=torch.Generator().manual_seed(3)).to(_dev())
    gp = render_nc_backward(*[t[perm].contiguous() for t in a], geo, lasers, cfg, G)
    assert all(torch.equal(x[perm], y) for x, y in zip(g1, gp))
    head = render_nc_backward(*[t[:17].contiguous() for t in a], geo, lasers, cfg, G)
    assert all(torch.equal(x[:17], y) for x, y in zip(g1, head))
    # one laser for the capture is the repeated spot
    one = lasers[1:2].contiguous()
    rep = one.expand(geo.nwall, 3).contiguous()
    ha, ga = _run(model, geo, one, cfg, G)
    hb, gb = _run(model, geo, rep, cfg, G)
    assert torch.equal(ha, hb) and all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert not torch.equal(ha, h1)


# ---------------------------------------------------------------------------------------------------------
# the confocal limit, the autograd front and the training step
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["cuda", "torch"])
def test_confocal_limit(preset):
    """lasers == sensors: the new kernels and the default confocal renderer are each within their tolerance of the
    same float64 reference (different kernels, different summation order: not bitwise)."""
    from nlosgr.render import render_backward, render_forward
    b = _base(preset)
    model, geo, gout = b["model"], b["geo"], b["gout"]
    lasers = geo.wall.clone()
    ref = NCO.reference(VO.params_of_model(model), geo, lasers, preset, 5.7, gout)
    want = VO.reference(VO.params_of_model(model), geo, preset, "noocl", 1.0, 5.7, gout)
    assert bool(((ref.hist - want.hist).abs() <= 1e-12 * want.hist.amax(dim=1, keepdim=True)).all())
    for n in VO.NAMES:   # (the same sums through another order of float64 operations)
        assert bool(((ref.grads[n] - want.grads[n]).abs().amax(dim=-1) <= 1e-10 * want.scale[n]).all()), n
    _judge(f"confocal limit {preset}", model, geo, lasers, preset, 5.7, gout, ref=ref)
    cfg = _cfg(preset, 5.7, 3)
    G = gout.to(_dev()).float().contiguous()
    h, _ = render_forward(*_args(model), geo, cfg)
    got = render_backward(*_args(model), geo, cfg, grad_hist=G)
    fwd, worst = VO.forward_worst(h, ref), VO.worst(VO.as_named(got), ref)
    print(f"confocal renderer against the same reference: forward {fwd:.2e}; "
          + ", ".join(f"{n} {v:.2e}" for n, v in worst.items()))
    assert fwd <= 2e-5 and max(worst.values()) <= 2e-4


def test_autograd_front():
    from nlosgr.render_nc import render_nc
    b = _base("cuda")
    a = [t.clone().requires_grad_(True) for t in _args(b["model"])]
    G = b["gout"].to(_dev()).float()
    h = render_nc(*a, b["geo"], b["lasers"], _cfg("cuda", 5.7, 3))
    (h * G).sum().backward()
    h2, got = _run(b["model"], b["geo"], b["lasers"], _cfg("cuda", 5.7, 3), G)
    assert torch.equal(h.detach(), h2)
    assert all(torch.equal(x.grad.reshape(y.shape), y) for x, y in zip(a, got))


def test_train_step(tmp_path):
    """NcTrainStep: step 1's gradients against float64 autograd through the oracle and the MSE; densify.relocate_gs
    and a rebind, a second step, and a checkpoint round trip."""
    from nlosgr import GaussianParams, densify
    from nlosgr.checkpoint import load_checkpoint, save_checkpoint
    from nlosgr.render_nc import NcTrainStep
    b = _base("cuda")
    src, geo, lasers = b["model"], b["geo"], b["lasers"]
    model = GaussianParams(*[t.detach().clone() for t in (src._mu, src._scaling, src._rotation, src._opacity,
                                                          src._features_dc, src._features_rest)], 3, 3)
    ref0 = _base_ref("cuda", 5.7)
    target = (0.5 * ref0.hist.flip(0)).float().to(_dev())          # another measurement's row: a large residual
    cfg = _cfg("cuda", 5.7, 3)
    step = NcTrainStep(model, geo, lasers, cfg, target, gt_times=1.5, keep_grads=True)
    P = VO.params_of_model(model)
    gout = 2.0 * (ref0.hist - 1.5 * target.cpu().double()) / ref0.hist.numel()       # dMSE/dhist in float64
    ref = NCO.reference(P, geo, lasers, "cuda", 5.7, gout)
    before = model._mu.detach().clone()
    loss2 = step()
    want_loss = float(((ref0.hist - 1.5 * target.cpu().double()) ** 2).mean())
    assert abs(float(loss2[0]) - want_loss) <= 1e-4 * want_loss
    g = step.grads                                                                   # train.GROUPS order
    named = VO.as_named([g[0], g[4], g[5], g[3].reshape(-1, 1), g[1], g[2]])
    worst = VO.worst(named, ref)
    print("\ntrain step: " + ", ".join(f"{n} {v:.2e}" for n, v in worst.items()))
    _TABLE["train step"] = dict(worst)
    bad = VO.failures(named, ref, TOL_G)
    assert not bad, bad[:6]
    assert step.iteration == 1 and not torch.equal(before, model._mu.detach())
    dead = torch.zeros(48, dtype=torch.bool, device=_dev())
    dead[3] = True
    densify.relocate_gs(model, dead, train_step=step)
    step.rebind()
    assert torch.isfinite(step()).all() and step.iteration == 2
    ck = str(tmp_path / "nc.pt")
    save_checkpoint(ck, model, train_step=step)
    saved = torch.load(ck, map_location="cpu", weights_only=True)
    assert saved["iteration"] == 2 and len(saved["optimizer"]["state"]) == 6
    back = load_checkpoint(ck, device=_dev())
    assert torch.equal(back._mu.detach(), model._mu.detach()) and torch.equal(back._opacity.detach(), model._opacity.detach())


def test_command_line(tmp_path):
    """python -m nlosgr.render_nc on a small non-confocal capture file (the base scene's own render as the data):
    the Gaussians come from the back-projection, and the checkpoint carries the step's Adam state."""
    import numpy as np
    from nlosgr.data import save_zaragoza
    from nlosgr.render_nc import main
    b = _base("cuda")
    geo, lasers = b["geo"], b["lasers"]
    rows = _run(b["model"], geo, lasers, _cfg("cuda", 5.7, 3)).cpu().numpy()           # [6, 97], bins 30 .. 126
    data = np.zeros((127, 2, 3), dtype=np.float32)
    data[30:127] = rows.T.reshape(97, 2, 3)
    path = str(tmp_path / "nc.mat")
    save_zaragoza(path, data, geo.wall.cpu().numpy().T.copy(), (0.0, 0.5, 0.0), 0.5, 8e-3, 1.0,
                  laser_grid_positions=lasers.cpu().numpy().T.copy())
    ck = str(tmp_path / "fit.pth")
    torch.manual_seed(2)
    np.random.seed(2)
    main([path, "--start", "30", "--end", "127", "--ns", "6", "--gaussians", "24", "--iterations", "3", "--cutoff", "5.7",
          "--resolution", "12", "--out", ck])
    saved = torch.load(ck, map_location="cpu", weights_only=True)
    assert saved["iteration"] == 3 and saved["mu"].shape == (24, 3) and len(saved["optimizer"]["state"]) == 6
    assert all(bool(torch.isfinite(saved[k]).all()) for k in ("mu", "scaling", "rotation", "opacity", "features_dc"))
