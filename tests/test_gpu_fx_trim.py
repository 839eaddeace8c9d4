"""Trimmed support of the no-occlusion fixed-point (FX) forward (FLAG_FX_TRIM; csrc/nlosgr_volume.hpp, fx_trim_m2).

That drain rounds every term to the nearest unit 2^-E, and a twin lane rounds the sum of two rays' terms, so a term
under a quarter unit adds exactly 0.  With the flag a (wall point, Gaussian) pair's support ends at the smaller of the
cutoff and the Mahalanobis radius m with m^2 = 2 ln 2 (lw + 2 + 2^-6), lw = log2(w 2^E), beyond which its value
is under a quarter unit (sin(theta) <= 1 ignored), and a pair that peaks under a quarter unit is skipped.  Fewer
passing cells pair up differently along their rows, so the trimmed histogram is not bitwise the untrimmed one; it
obeys the same bounds.  The small scene of tests/test_gpu_fx_runs.py (its helpers are used): 1500 Gaussians, seed 21,
3 x 3 wall, 256 bins, ns 16, 5.7 sigma, cuda preset; tolerance 2e-5 of each row's maximum.  Figures are printed
(pytest -s).
"""
import math
from dataclasses import replace

import pytest
import torch

from conftest import ROOT  # noqa: F401

import volume_oracle as VO
from test_gpu_fx_runs import CUT, TOL, _chunk_sum, _fx, _params, _row_err, _scene, _setup

pytestmark = pytest.mark.gpu

TRIM_MARGIN = 2.0 ** -6           # kTrimMargin
K_TRIM = 2.0 * math.log(2.0)      # kTrim


def _flags():
    from nlosgr import _lib
    return _lib.FLAG_FX_TRIM, _lib.FLAG_FX_NOTWIN


_SHARED = {}


def _small():
    """The small scene with its reference and its untrimmed default forward, computed once."""
    if not _SHARED:
        _, P, geo, cfg = _setup(_scene())
        _SHARED.update(P=P, geo=geo, cfg=cfg, ref=_chunk_sum(P, geo, cfg), plain=_fx(P, geo, cfg))
    return _SHARED


def test_trimmed_vs_references():
    """The trimmed default drain, the trimmed one-ray drain, the untrimmed default drain and the float64 sum of fp32
    float-drain sub-histograms agree pairwise within 2e-5 of each row's maximum; two trimmed runs are equal bit for
    bit with equal counts; the trimmed drain forms fewer groups than the untrimmed one (it dropped rays)."""
    TRIM, NOTWIN = _flags()
    s = _small()
    P, geo, cfg, ref = s["P"], s["geo"], s["cfg"], s["ref"]
    u, iu = s["plain"]
    a, ia = _fx(P, geo, cfg, TRIM)
    a2, ia2 = _fx(P, geo, cfg, TRIM)
    b, ib = _fx(P, geo, cfg, TRIM | NOTWIN)
    errs = {"trim/ref": _row_err(a, ref), "trim1/ref": _row_err(b, ref), "plain/ref": _row_err(u, ref),
            "trim/trim1": _row_err(a, b.double()), "trim/plain": _row_err(a, u.double()),
            "trim1/plain": _row_err(b, u.double())}
    print(f"\ntrim: E {ia[0]}, groups {ia[4]} (untrimmed {iu[4]}), splits {ia[5]} ({iu[5]}); "
          + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert ia[0] == iu[0] and ia[4] > 0 and ib[4] == 0 and ib[5] == 0, (ia, ib, iu)
    assert all(v <= TOL for v in errs.values()), errs
    assert torch.equal(a, a2) and ia == ia2
    assert ia[4] < iu[4], (ia, iu)


def _one_gaussian(dev):
    """One wall point at the origin and one Gaussian (sigma 0.05, 10 bins) straight in front of it in x, whose
    amplitude bound is 2^20 times its albedo: an l = 1 coefficient of 2e6 on the basis function that vanishes in
    the plane x = 0, found with the oracle.  The view direction has x = 0 exactly, so that term is exactly 0 in
    fp32 and in float64, the albedo is 0.5 exactly, and the values are a few units: their fp32 evaluation error
    (4e-5 relative at most, tests/test_gpu_fwd_edges.py) is below 1e-3 of the half unit per term that the bound
    allows, so the bound measures the rounding and the dropped terms and nothing else."""
    from nlosgr import GaussianParams
    from nlosgr.volume import Scene, make_config
    from oracle import torch_ref as R
    scene = Scene(H=1, W=1, T=256, ns=16)
    m = GaussianParams.synthetic(1, 3, preset="cuda", device=dev, seed=21)
    wall = scene.walls(torch.device("cpu"))[0]
    assert float(wall[0]) == 0.0
    with torch.no_grad():
        m._mu[:] = torch.tensor([[0.0, 0.5, 0.03]], device=dev)
        m._scaling[:] = math.log(0.05)
        m._rotation[:] = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev)
        m._opacity[:] = 0.0
        m._features_dc[:] = 0.0
        m._features_rest[:] = 0.0
        slot = None
        for c in range(3):       # the l = 1 slot whose basis function is 0 for this view direction
            m._features_rest[:] = 0.0
            m._features_rest[0, c, 0] = 2e6
            if float(R.albedo(VO.Params64(VO.params_of_model(m)), wall.double(), "cuda")[0, 0].detach()) == 0.5:
                slot = c
                break
        assert slot is not None, "no l = 1 basis function vanishes in the plane x = 0"
    geo = scene.geometry(dev, "cuda", "noocl")
    return m, geo, make_config(m, scene, "cuda", "noocl", cutoff=CUT)


@pytest.mark.parametrize("trimmed", [True, False])
def test_one_gaussian_per_bin_in_units(trimmed):
    """|hist 2^E / (att hscale) - exact| <= 0.5 n(bin) (1 + 1e-3) units, n(bin) = the rays whose full-cutoff
    support covers the bin and exact = their float64 sum: one rounding of at most half a unit per ray and bin (a twin
    rounds two rays' sum once).  A dropped term is under a quarter unit, so it stays inside its ray's half unit."""
    TRIM, _ = _flags()
    dev = torch.device("cuda:0")
    m, geo, cfg = _one_gaussian(dev)
    h, info = _fx(_params(m), geo, cfg, TRIM if trimmed else 0)
    E = info[0]
    assert info[3] == 0 and info[2] == 0, info
    P64 = VO.Params64(VO.params_of_model(m))
    tab = VO.tables(geo)
    with torch.no_grad():
        t = VO.ray_terms(P64, tab, 0, "cuda", "noocl", cfg.c_deltaT, CUT)[0]      # [nr, rays], x att hscale
    unit = (tab["hscale"][0] * tab["att"]).double() * 2.0 ** -E                     # one unit's worth per bin
    n = (t > 0).sum(dim=1).double()
    exact = t.sum(dim=1) / unit
    got = h[0].detach().cpu().double() / unit
    peak = float((t / unit[:, None]).max())
    err = (got - exact).abs()
    bound = 0.5 * n * (1.0 + 1e-3)
    lw = math.log2(0.5 * 0.5) + E      # sigma 0.5, albedo 0.5
    m_pair = math.sqrt(min(CUT * CUT, K_TRIM * (lw + 2.0 + TRIM_MARGIN)))
    worst = float((err / bound.clamp_min(1e-300))[n > 0].max())
    print(f"\none Gaussian ({'trimmed' if trimmed else 'untrimmed'}): E {E}, peak {peak:.2f} units, m_pair {m_pair:.2f} "
          f"sigma, n <= {int(n.max())}, groups {info[4]}; worst err / bound {worst:.3f}, "
          f"max err {float(err.max()):.3f} units, err where n = 0: {float(err[n == 0].max()) if bool((n == 0).any()) else 0.0:.3e}")
    assert 1.0 <= peak <= 16.0 and m_pair < 0.6 * CUT, "the scene no longer trims deep inside the cutoff"
    assert float(got.sum()) > 0.0
    assert bool((err <= bound).all()), [(int(k), float(err[k]), float(bound[k])) for k in torch.nonzero(err > bound)[:6, 0]]


def test_dim_pairs_vanish_exactly():
    """One ordinary Gaussian and 63 copies of it at opacity -20: the unit is the ordinary one's, and every copy peaks
    under a quarter unit at every wall point (checked here on the CPU with the oracle's albedo).  Trimmed, the
    histogram is bitwise the ordinary Gaussian's alone, with equal group and split counts; untrimmed, the copies'
    rays form groups of their own."""
    from oracle import torch_ref as R
    TRIM, _ = _flags()
    m, P, geo, cfg = _setup(_scene())
    one = [t[:1].contiguous() for t in P]
    many = [t[:1].repeat(64, *([1] * (t.dim() - 1))).contiguous() for t in P]
    many[3][1:] = -20.0
    alone, i1 = _fx(one, geo, cfg, TRIM)
    E = i1[0]
    Pm = VO.Params64(R.Params(*[t[:1].detach().cpu() for t in (m._mu, m._scaling, m._rotation, m._opacity,
                                                               m._features_dc, m._features_rest)],
                              int(m.active_sh_degree), requires_grad=False))
    with torch.no_grad():
        rho = max(float(R.albedo(Pm, geo.wall[p].detach().cpu().double(), "cuda")[0, 0]) for p in range(geo.nwall))
    sig = float(torch.sigmoid(torch.tensor(-20.0, dtype=torch.float32)))
    peak = sig * rho * 2.0 ** E
    a, ia = _fx(many, geo, cfg, TRIM)
    u, iu = _fx(many, geo, cfg)
    print(f"\ndim pairs: E {E}, a copy peaks at {peak:.3e} units; groups alone {i1[4]}, trimmed {ia[4]}, "
          f"untrimmed {iu[4]}; splits {i1[5]} / {ia[5]} / {iu[5]}")
    assert rho > 0 and peak * 1.001 < 0.25 * 2.0 ** -TRIM_MARGIN, peak
    assert ia[0] == E and iu[0] == E
    assert float(alone.sum()) > 0.0 and i1[4] > 0
    assert torch.equal(a, alone) and ia[4] == i1[4] and ia[5] == i1[5], (ia, i1)
    assert iu[4] > i1[4], (iu, i1)


def test_no_trimming_above_the_cutoff():
    """Opacity 4 and albedo 1 with no SH rest (volume_oracle.tight_albedo): every bound is 1.03 sigma, so every pair
    has lw >= 22.9 and its quarter-unit radius, 2 ln 2 (lw + 2 + 2^-6) >= 34.5, lies beyond 5.7^2 = 32.49 (checked
    here from E): the trimmed forward is bitwise the untrimmed one."""
    TRIM, _ = _flags()
    def bright(mm):
        VO.tight_albedo(mm, opacity=4.0)
    _, P, geo, cfg = _setup(_scene(), edit=bright)
    u, iu = _fx(P, geo, cfg)
    a, ia = _fx(P, geo, cfg, TRIM)
    lw = math.log2(float(torch.sigmoid(torch.tensor(4.0))) * 1.0) + iu[0]
    print(f"\nabove the cutoff: E {iu[0]}, lw {lw:.2f}, quarter-unit radius^2 {K_TRIM * (lw + 2 + TRIM_MARGIN):.2f} "
          f"vs {CUT * CUT:.2f}; groups {ia[4]}, bright segments {ia[3]}")
    assert K_TRIM * (lw + 2.0 + TRIM_MARGIN) > CUT * CUT * 1.001
    assert float(u.sum()) > 0.0
    assert torch.equal(a, u) and ia == iu, (ia, iu)


def _thin(m):
    m._scaling[:, 1] = math.log(3e-4)


@pytest.mark.parametrize("case", ["ns5", "T41", "thin"])
def test_edges(case):
    """The trimmed forward on ns 5 (boxes narrower than a trip), on 41 bins clipped at both ends and on Gaussians
    with one 3e-4 axis (groups split at the merge guard), each against the float64 sum of float-drain
    sub-histograms, the untrimmed default drain and the trimmed one-ray drain within 2e-5 of each row's maximum."""
    TRIM, NOTWIN = _flags()
    scene = {"ns5": _scene(ns=5), "T41": _scene(T=41, start=90, deltaT=5e-3), "thin": _scene()}[case]
    _, P, geo, cfg = _setup(scene, edit=_thin if case == "thin" else None)
    ref = _chunk_sum(P, geo, cfg)
    a, ia = _fx(P, geo, cfg, TRIM)
    b, _ = _fx(P, geo, cfg, TRIM | NOTWIN)
    u, iu = _fx(P, geo, cfg)
    errs = (_row_err(a, ref), _row_err(b, ref), _row_err(a, u.double()), _row_err(a, b.double()))
    print(f"\ntrim {case}: groups {ia[4]} (untrimmed {iu[4]}), splits {ia[5]} ({iu[5]}); vs ref {errs[0]:.3e}, one-ray vs "
          f"ref {errs[1]:.3e}, vs untrimmed {errs[2]:.3e}, vs one-ray {errs[3]:.3e}")
    assert float(a.sum()) > 0.0 and torch.isfinite(a).all() and float(a.min()) >= 0.0
    if case == "T41":
        assert geo.nr == 41 and float(a[:, 0].min()) > 0.0 and float(a[:, -1].min()) > 0.0, "nothing was clipped"
    if case == "thin":
        assert iu[5] > 0, iu
    assert max(errs) <= TOL, errs


def test_no_gaussians():
    """No Gaussian at all: the trimmed forward ends and the histogram is zero."""
    from nlosgr.render import render_forward
    TRIM, _ = _flags()
    s = _small()
    h, _ = render_forward(*[t[:0].contiguous() for t in s["P"]], s["geo"], replace(s["cfg"], flags=TRIM))
    torch.cuda.synchronize()
    assert h.shape == (s["geo"].nwall, s["geo"].nr) and float(h.abs().max()) == 0.0
