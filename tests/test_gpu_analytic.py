"""GPU parity of the analytic paths against the CPU oracle.

Path A (nlosgr_rays_analytic, the reference's _C.render_rays_analytic):
    per-ray value   max|hip - ref| <= 1e-5 * max|ref| + 1e-7   (fp32, same filter rows)
C4 "analytic_exact" (mode "binint" of the volume forward: exact per-bin erf average):
    hist            max|hip - ref| <= 5e-5 * max|ref| + 1e-9   (fp32 erfc vs the float64 oracle)
and the C4 cross-check: binint vs the point-sampled numerical path differs by the bin-averaging
term only, relative L2 <= (dr/sigma_r)^2 / 24 * 4 for the sizes used (stated below).
"""
import math

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu


def _close(a, b, rtol, atol, msg=""):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = np.abs(b).max() if b.size else 0.0
    err = np.abs(a - b).max() if b.size else 0.0
    assert err <= rtol * scale + atol, f"{msg}: max err {err:.3e} vs scale {scale:.3e}"


def _oracle_params(model, deg):
    from oracle import torch_ref as R
    cpu = lambda t: t.detach().cpu()
    return R.Params(cpu(model._mu), cpu(model._scaling), cpu(model._rotation), cpu(model._opacity),
                    cpu(model._features_dc), cpu(model._features_rest), deg, requires_grad=False)


def _ray_grid(cam, nt, nph, dev):
    th = torch.linspace(0.35, 1.3, nt, device=dev)
    ph = torch.linspace(1.0, 2.2, nph, device=dev)
    tg, pg = torch.meshgrid(th, ph, indexing="ij")
    tf, pf = tg.reshape(-1), pg.reshape(-1)
    d = torch.stack([torch.sin(tf) * torch.cos(pf), torch.sin(tf) * torch.sin(pf), torch.cos(tf)], 1).contiguous()
    o = cam.unsqueeze(0).expand(d.shape[0], 3).contiguous()
    return o, d


@pytest.mark.parametrize("deg,ng,shift,opac", [(0, 60, 0.8, 0.0), (3, 300, 1.6, 2.0), (1, 40, 2.5, 6.0)])
def test_rays_analytic_vs_oracle(deg, ng, shift, opac):
    """Per-ray analytic value vs the restatement of volume_renderer_analytic.cu, same filter rows.
    Case 2 has > 128 sections on many rays (cap), case 3 opaque Gaussians (early exit)."""
    from nlosgr import GaussianParams, features_flat
    from nlosgr.rays import filter_gaussians_per_ray, render_rays_analytic
    from nlosgr.render import bboxes
    from oracle import torch_ref as R
    dev = torch.device("cuda:0")
    m = GaussianParams.synthetic(ng, deg, preset="cuda", device=dev, seed=11 + deg)
    with torch.no_grad():
        m._scaling.add_(shift)
        m._opacity.add_(opac)
    cam = torch.tensor([0.05, 0.0, -0.1], device=dev)
    o, d = _ray_grid(cam, 12, 10, dev)
    bb = bboxes(m._mu, m._scaling, m._rotation, 1.0, 3.0, preset="torch")
    filt = filter_gaussians_per_ray(o, d, m._mu, bb.view(-1, 6), 3.0)
    feats = features_flat(m)
    t0, t1 = 0.16, 1.44
    out = render_rays_analytic(o, d, t0, t1, filt, m._mu, m._scaling, m._rotation, m._opacity, feats, cam, deg,
                               1.0, 1.28 / 64, 1.0, 3.0)
    P = _oracle_params(m, deg)
    ref = R.render_rays_analytic(o.cpu(), d.cpu(), t0, t1, filt.cpu(), P, feats.detach().cpu(), cam.cpu(), deg)
    if ng >= 300:
        assert int(filt[:, 0].max()) > 128
    assert ref.abs().max() > 0
    _close(out.cpu(), ref, 1e-5, 1e-7, "analytic per-ray vs the fp32 restatement")
    ref64 = R.render_rays_analytic_batched(o.cpu(), d.cpu(), t0, t1, filt.cpu(), P, feats.detach().cpu(), cam.cpu(),
                                           deg, dtype=torch.float64)
    _close(out.cpu(), ref64, 1e-5, 0.0, "analytic per-ray vs the formula in float64")


def _clear_hits(o, d, P, t0, t1, sigma=3.0):
    """bool [nrays, Ng] in float64: the ray's line crosses the Gaussian's sigma-ellipsoid and the clipped section
    is non-empty, both by a margin fp32 cannot close (so a row made of such Gaussians has exactly that many
    sections in the kernel too)."""
    from oracle import torch_ref as R
    mu, s = P._mu.double(), torch.exp(P._scaling.double())
    Rt = R.quat_to_rotmat_cuda(P._rotation.double()).transpose(1, 2)
    so = torch.einsum("gab,rgb->rga", Rt, o.double()[:, None, :] - mu[None]) / s[None]
    sd = torch.einsum("gab,rb->rga", Rt, d.double()) / s[None]
    a, b, cc = (sd * sd).sum(-1), 2.0 * (so * sd).sum(-1), (so * so).sum(-1) - sigma * sigma
    disc = b * b - 4.0 * a * cc
    sq = torch.sqrt(disc.clamp_min(0.0))
    te, tx = ((-b - sq) / (2.0 * a)).clamp_min(t0), ((-b + sq) / (2.0 * a)).clamp_max(t1)
    return (disc > 1e-3 * (b * b + 4.0 * a * cc.abs())) & (tx - te > 1e-3)


def test_rays_analytic_section_cap_and_ties():
    """analytic_kernel at its edges, against the formula in float64 at 1e-5: nrays 5 and 1 (4 rays per workgroup);
    a ray with exactly 128 sections (kMaxSec) and one with 129, whose last one the cap drops; two identical
    Gaussians on one ray, whose equal t_enter must rank by filter order (a rank collision would lose a section).
    The Gaussians are faint (opacity - 4), so no ray reaches the early exit and every section counts."""
    from nlosgr import GaussianParams, features_flat
    from nlosgr.rays import render_rays_analytic
    from oracle import torch_ref as R
    dev = torch.device("cuda:0")
    deg, ng = 2, 220
    m = GaussianParams.synthetic(ng, deg, preset="cuda", device=dev, seed=17)
    with torch.no_grad():
        m._scaling.add_(1.0)
        m._opacity.add_(-4.0)
        for t in (m._mu, m._scaling, m._rotation, m._opacity, m._features_dc, m._features_rest):
            t[131] = t[130]                      # two identical Gaussians
    cam = torch.tensor([0.05, 0.0, -0.1], device=dev)
    o, d = _ray_grid(cam, 5, 1, dev)
    P = _oracle_params(m, deg)
    feats = features_flat(m)
    t0, t1 = 0.16, 1.44
    hit = _clear_hits(o.cpu(), d.cpu(), P, t0, t1)
    assert bool(hit[2, 130]) and bool(hit[2, 131])
    lists = [torch.nonzero(hit[0]).flatten()[:128].tolist(), torch.nonzero(hit[1]).flatten()[:129].tolist(),
             [int(torch.nonzero(hit[2]).flatten()[0]), 130, 131, int(torch.nonzero(hit[2]).flatten()[-1])],
             torch.nonzero(hit[3]).flatten()[::3].tolist(), []]
    assert [len(x) for x in lists[:3]] == [128, 129, 4]
    filt = torch.full((5, 257), -1, dtype=torch.int32)
    for r, idx in enumerate(lists):
        filt[r, 0] = len(idx)
        filt[r, 1:1 + len(idx)] = torch.tensor(idx, dtype=torch.int32)

    def ref64(f, rays=slice(None)):
        return R.render_rays_analytic_batched(o.cpu()[rays], d.cpu()[rays], t0, t1, f, P, feats.detach().cpu(), cam.cpu(),
                                              deg, dtype=torch.float64)

    def hip(f, rays=slice(None)):
        return render_rays_analytic(o[rays].contiguous(), d[rays].contiguous(), t0, t1, f.to(dev), m._mu, m._scaling,
                                    m._rotation, m._opacity, feats, cam, deg, 1.0, 1.28 / 64, 1.0, 3.0).cpu()

    ref = ref64(filt)
    # the reference sees what the case is about: the 128th section counts, the 129th is dropped, and the second of
    # the identical Gaussians adds a section of its own
    cut = filt.clone()
    cut[0, 0], cut[1, 0], cut[2, 0] = 127, 128, 2
    rc = ref64(cut)
    assert abs(float(ref[0] - rc[0])) > 1e-4 * float(ref[0]) and float(ref[1]) == float(rc[1])   # 10 x the tolerance
    assert abs(float(ref[2] - rc[2])) > 1e-2 * float(ref[2]) and float(ref[4]) == 0.0
    out = hip(filt)
    assert float(out[4]) == 0.0
    _close(out, ref, 1e-5, 0.0, "analytic, 5 rays")
    for r in range(3):                      # nrays = 1: each ray against its own value
        one = hip(filt[r:r + 1].contiguous(), slice(r, r + 1))
        assert one.shape == (1,)
        _close(one, ref[r:r + 1], 1e-5, 0.0, f"analytic ray {r} alone")
        assert float(one[0]) == float(out[r])


def test_section_renderer_dropin():
    """SectionGaussianRendererCUDA.render_transient: middle-bin placement and broadcast histogram
    (section_renderer.py:163-184) around the per-ray values."""
    from nlosgr import GaussianParams
    from nlosgr.rendering_section import create_section_renderer
    from nlosgr.rays import filter_gaussians_per_ray
    from nlosgr.render import bboxes
    from oracle import torch_ref as R
    dev = torch.device("cuda:0")
    m = GaussianParams.synthetic(80, 0, preset="cuda", device=dev, seed=2)
    with torch.no_grad():
        m._scaling.add_(1.0)
    cam = torch.tensor([0.0, 0.0, 0.0], device=dev)
    rend = create_section_renderer(3.0)
    assert rend is not None
    th_r, ph_r, nt, nph, nr = (0.3, 1.4), (0.9, 2.3), 8, 6, 20
    result, hist = rend.render_transient(m, cam, th_r, ph_r, (0.16, 1.44), nt, nph, nr, 1.0, 0.02)
    assert result.shape == (nr, nt, nph) and hist.shape == (nr,)
    assert torch.count_nonzero(result[torch.arange(nr) != nr // 2]) == 0
    th = torch.linspace(*th_r, nt)
    ph = torch.linspace(*ph_r, nph)
    tg, pg = torch.meshgrid(th, ph, indexing="ij")
    tf, pf = tg.reshape(-1), pg.reshape(-1)
    d = torch.stack([torch.sin(tf) * torch.cos(pf), torch.sin(tf) * torch.sin(pf), torch.cos(tf)], 1)
    o = torch.zeros_like(d)
    bb = bboxes(m._mu, m._scaling, m._rotation, 1.0, 3.0, preset="torch").view(-1, 6)
    filt = filter_gaussians_per_ray(o.to(dev), d.to(dev).contiguous(), m._mu, bb, 3.0).cpu()
    P = _oracle_params(m, 0)
    ref = R.render_rays_analytic(o, d, 0.16, 1.44, filt, P, P.features[:, :, 0], cam.cpu(), 0)
    _close(result[nr // 2].cpu().reshape(-1), ref, 1e-5, 1e-7, "mid bin")
    expect = ref.sum() * (th_r[1] - th_r[0]) / nt * (ph_r[1] - ph_r[0]) / nph
    np.testing.assert_allclose(hist.cpu().numpy(), np.full(nr, expect.item()), rtol=1e-5)


@pytest.mark.parametrize("preset", ["cuda", "torch"])
@pytest.mark.parametrize("cutoff", [0.0, 3.0, 5.7])
def test_binint_volume_vs_oracle(preset, cutoff):
    """Bin-integrated forward (mode "binint") vs the float64 oracle, same support rule (at cutoff >= 5
    the TAIL drain: the series bin average for rays wider than 1.4 bins, erf differences below)."""
    from nlosgr import GaussianParams, features_flat
    from nlosgr.geometry import build_geometry, relay_wall_grid, volume_box_point
    from nlosgr.render import RenderConfig, render_forward
    from oracle import torch_ref as R
    dev = torch.device("cuda:0")
    ng, deg, ns, T = 40, 3, 6, 48
    c, deltaT = 1.0, 1.28 / T
    start, end = T // 8, T // 8 + T
    m = GaussianParams.synthetic(ng, deg, preset=preset, device=dev, seed=5)
    if preset == "cuda":
        with torch.no_grad():
            m._scaling.add_(1.2)
    walls = relay_wall_grid(2, 2, device=dev)
    box = volume_box_point((0.0, 0.5, 0.0), 0.5, dev)
    geo = build_geometry(walls, box, ns, start, end, c, deltaT, 0.5, preset, "binint")
    cfg = RenderConfig(preset=preset, mode="binint", sh_degree=deg, cutoff=cutoff, c_deltaT=c * deltaT)
    hist, _ = render_forward(m._mu, m._scaling, m._rotation, m._opacity, features_flat(m), geo, cfg)
    P = _oracle_params(m, deg)
    ref = R.render_volume_binint(P, walls.cpu(), box.cpu(), 0.5, ns, start, end, c, deltaT, preset,
                                 mc=cutoff if cutoff > 0 else None)
    _close(hist.cpu(), ref, 5e-5, 1e-9, f"binint {preset} mc={cutoff}")


@pytest.mark.parametrize("shift", [-2.5, 0.0, 1.2])
def test_binint_tail_series_and_erf_rays(shift):
    """The binint TAIL drain (cutoff 5.7) on Gaussians from sub-bin (every ray on the erf path) through
    mixed rounds to many bins wide (series path) vs the float64 oracle (T = 96)."""
    from nlosgr import GaussianParams, features_flat
    from nlosgr.geometry import build_geometry, relay_wall_grid, volume_box_point
    from nlosgr.render import RenderConfig, render_forward
    from oracle import torch_ref as R
    dev = torch.device("cuda:0")
    ng, deg, ns, T = 40, 3, 6, 96
    c, deltaT = 1.0, 1.28 / T
    start, end = T // 8, T // 8 + T
    m = GaussianParams.synthetic(ng, deg, preset="cuda", device=dev, seed=8)
    with torch.no_grad():
        m._scaling.add_(shift + 0.6 * torch.randn(m._scaling.shape, generator=torch.Generator().manual_seed(1)).to(dev))
    walls = relay_wall_grid(2, 2, device=dev)
    box = volume_box_point((0.0, 0.5, 0.0), 0.5, dev)
    geo = build_geometry(walls, box, ns, start, end, c, deltaT, 0.5, "cuda", "binint")
    cfg = RenderConfig(preset="cuda", mode="binint", sh_degree=deg, cutoff=5.7, c_deltaT=c * deltaT)
    hist, _ = render_forward(m._mu, m._scaling, m._rotation, m._opacity, features_flat(m), geo, cfg)
    P = _oracle_params(m, deg)
    ref = R.render_volume_binint(P, walls.cpu(), box.cpu(), 0.5, ns, start, end, c, deltaT, "cuda", mc=5.7)
    assert float(ref.abs().max()) > 0
    _close(hist.cpu(), ref, 5e-5, 1e-9, f"binint TAIL shift {shift}")


def test_binint_backward_unsupported():
    from nlosgr import GaussianParams, features_flat
    from nlosgr.volume import Scene, make_config
    from nlosgr.render import render_backward
    dev = torch.device("cuda:0")
    scene = Scene(H=2, W=2, T=32, ns=4)
    m = GaussianParams.synthetic(8, 0, preset="cuda", device=dev, seed=1)
    geo = scene.geometry(dev, "cuda", "binint")
    cfg = make_config(m, scene, mode="binint", cutoff=3.0)
    with pytest.raises(RuntimeError, match="bin-integrated"):
        render_backward(m._mu, m._scaling, m._rotation, m._opacity, features_flat(m), geo, cfg,
                        grad_hist=torch.ones(4, 32, device=dev))


def test_binint_vs_numerical_crosscheck():
    """C4 cross-check at reduced size: the bin average differs from the point sample by
    ~ (dr^2 a / 24)(1 - kap^2 a dr^2) per ray, so the volume-level relative L2 is bounded by
    ~ (dr / sigma_r)^2 / 24 with sigma_r >= s_min; the test allows 4x that bound."""
    from nlosgr import GaussianParams
    from nlosgr.volume import Scene, make_config, render_volume
    dev = torch.device("cuda:0")
    scene = Scene(H=8, W=8, T=512, ns=32)
    m = GaussianParams.synthetic(5000, 3, preset="cuda", device=dev, seed=9)
    geo_n = scene.geometry(dev, "cuda", "noocl")
    geo_b = scene.geometry(dev, "cuda", "binint")
    with torch.no_grad():
        h_num = render_volume(m, geo_n, make_config(m, scene, mode="noocl", cutoff=5.0))
        h_bin = render_volume(m, geo_b, make_config(m, scene, mode="binint", cutoff=5.0))
    rel = ((h_bin - h_num).norm() / h_num.norm()).item()
    dr = 1.28 / 512 * 512 / 511
    s_min = torch.exp(m._scaling).min().item()
    bound = 4 * (dr / s_min) ** 2 / 24
    assert 0 < rel < bound, (rel, bound)


def test_path_a_at_c4_scale():
    """Path A (nlosgr_rays_analytic = _C.render_rays_analytic, volume_renderer_analytic.cu:23-241) on
    the C3/C4 inputs: all 100k Gaussians, the full 32x32 ray grids of 4 wall points (angular ranges
    of spherical_sample_histogram, t range (I1, I2) c dT), per-ray 3-sigma box filter with the
    256-entry cap, 128-section cap, early exit.  Every ray's value against the vectorised oracle
    restatement fed the same filter rows (the filter itself is bit-exact vs the oracle's, see
    test_gpu_rays.py::test_filter_matches_oracle), evaluated in float64: at C3's Gaussian sizes tau is
    ~1e-7 per section, where the reference formula's fp32 1 - exp(-tau) is pure cancellation (the
    kernel uses -expm1(-tau)); tolerance 1e-4 of the largest ray value."""
    from nlosgr import GaussianParams, features_flat
    from nlosgr.rays import filter_gaussians_per_ray, render_rays_analytic
    from nlosgr.render import bboxes
    from nlosgr.volume import Scene
    from oracle import torch_ref as R
    dev = torch.device("cuda:0")
    scene = Scene(H=128, W=128, T=1024, ns=32)
    m = GaussianParams.synthetic(100_000, 3, preset="cuda", device=dev, seed=0)
    geo = scene.geometry(dev, "cuda", "noocl")
    feats = features_flat(m)
    bb = bboxes(m._mu, m._scaling, m._rotation, 1.0, 3.0, preset="torch").view(-1, 6)
    P = _oracle_params(m, 3)
    t0, t1 = float(geo.r[0]), float(geo.r[-1])
    capped = 0
    for p in (0, 128 * 40 + 30, 128 * 64 + 64, 128 * 127 + 100):
        th, ph = geo.theta[p], geo.phi[p]
        tg, pg = torch.meshgrid(th, ph, indexing="ij")
        tf, pf = tg.reshape(-1), pg.reshape(-1)
        d = torch.stack([torch.sin(tf) * torch.cos(pf), torch.sin(tf) * torch.sin(pf), torch.cos(tf)], 1).contiguous()
        cam = geo.wall[p].contiguous()
        o = cam.unsqueeze(0).expand(d.shape[0], 3).contiguous()
        filt = filter_gaussians_per_ray(o, d, m._mu, bb, 3.0)
        out = render_rays_analytic(o, d, t0, t1, filt, m._mu, m._scaling, m._rotation, m._opacity, feats, cam, 3,
                                   1.0, 1.28 / 1024, 1.0, 3.0)
        assert out.shape == (1024,) and torch.isfinite(out).all()
        capped += int((filt[:, 0] >= 256).sum())
        ref = R.render_rays_analytic_batched(o.cpu(), d.cpu(), t0, t1, filt.cpu(), P, feats.detach().cpu(), cam.cpu(), 3,
                                             dtype=torch.float64)
        assert ref.abs().max() > 0
        _close(out.cpu(), ref, 1e-4, 0.0, f"path A wall point {p}")
    assert capped > 0   # the reference's 256-entry truncation is exercised at this density
