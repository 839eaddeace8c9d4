"""The twin drain of the no-occlusion fixed-point (FX) forward (csrc/nlosgr_volume_fwd.hip, fx_twin_setup).

By default a lane of the FX drain takes two adjacent rays (i, j), (i, j + 1) of one (wall point, Gaussian) pair,
walks the union of their bin ranges and adds the two values of every bin with one LDS atomic;
FLAG_FX_NOTWIN selects the single-segment drain (one ray per lane).  These tests pin the twin drain against
the float64 sum of fp32 FLAG_FLOAT_DRAIN sub-histograms of 250 Gaussians each (the reference of
tests/test_gpu_fx.py, and its tolerance: 2e-5 of each row's maximum), against the single-segment drain, and
its merge guard (a twin whose second ray's recurrence could not be seeded at the union's first bin is split
and drained as two segments).  All at the cuda preset, no occlusion, 5.7 sigma.  The measured figures are
printed (pytest -s).
"""
import math
from dataclasses import replace

import pytest
import torch

from conftest import ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

CUT = 5.7
TOL = 2e-5
NG = 1500


def _params(m):
    from nlosgr import features_flat
    return [m._mu.detach(), m._scaling.detach(), m._rotation.detach(), m._opacity.detach(),
            features_flat(m).detach().contiguous()]


def _chunk_sum(P, geo, cfg, chunk=250):
    """float64 sum of fp32 float-drain sub-histograms of `chunk` Gaussians each."""
    from nlosgr import _lib
    from nlosgr.render import render_forward
    fcfg = replace(cfg, flags=_lib.FLAG_FLOAT_DRAIN)
    ref = torch.zeros(geo.nwall, geo.nr, dtype=torch.float64, device=P[0].device)
    for g0 in range(0, P[0].shape[0], chunk):
        h, _ = render_forward(*[t[g0:g0 + chunk].contiguous() for t in P], geo, fcfg)
        ref += h.double()
    return ref


def _fx(P, geo, cfg, flags=0):
    """(histogram, (E, E max, flushes, bright segments, twins, splits)) of one FX forward."""
    from nlosgr.render import fx_info, render_forward, workspace_for
    c = replace(cfg, flags=flags)
    ws = workspace_for(*P, geo, c)
    h, _ = render_forward(*P, geo, c, workspace=ws)
    return h, fx_info(*P, geo, c, ws)


def _row_err(a, ref):
    return float(((a.double() - ref).abs().max(1).values / ref.abs().max(1).values).max())


def _setup(scene, seed=21, edit=None):
    from nlosgr import GaussianParams
    from nlosgr.volume import make_config
    dev = torch.device("cuda:0")
    m = GaussianParams.synthetic(NG, 3, preset="cuda", device=dev, seed=seed)
    if edit is not None:
        with torch.no_grad():
            edit(m)
    P = _params(m)
    geo = scene.geometry(dev, "cuda", "noocl")
    cfg = make_config(m, scene, "cuda", "noocl", cutoff=CUT)
    return P, geo, cfg


def _scene(T=256, **kw):
    from nlosgr.volume import Scene
    return Scene(H=3, W=3, T=T, ns=16, **kw)


def test_twin_vs_single_vs_reference():
    """1500 synthetic Gaussians on a 3 x 3 wall: the twin drain and the single-segment drain each within
    2e-5 of the reference and of each other; twins were formed and none split; two default runs are equal
    bit for bit (integer sums)."""
    from nlosgr import _lib
    P, geo, cfg = _setup(_scene())
    ref = _chunk_sum(P, geo, cfg)
    a, ia = _fx(P, geo, cfg)
    a2, ia2 = _fx(P, geo, cfg)
    b, ib = _fx(P, geo, cfg, _lib.FLAG_FX_NOTWIN)
    ea, eb, eab = _row_err(a, ref), _row_err(b, ref), _row_err(a, b.double())
    print(f"\ntwin: twins {ia[4]}, splits {ia[5]}; twin vs ref {ea:.3e}, single vs ref {eb:.3e}, "
          f"twin vs single {eab:.3e} (of each row's max)")
    assert ia[4] > 0 and ia[5] == 0, ia
    assert ib[4] == 0 and ib[5] == 0, ib
    assert ea <= TOL and eb <= TOL and eab <= TOL
    assert torch.equal(a, a2) and ia == ia2


def test_twin_narrow_gaussians_split():
    """One axis of every Gaussian 3e-4 long (5.7 sigma is a third of the 5e-3 bin): along a ray the Gaussian is
    under one bin wide, adjacent rays meet it more than its width apart, so the merge guard splits twins; the
    result stays finite, non-negative and within tolerance."""
    def thin(m):
        m._scaling[:, 1] = math.log(3e-4)
    P, geo, cfg = _setup(_scene(), edit=thin)
    ref = _chunk_sum(P, geo, cfg)
    a, ia = _fx(P, geo, cfg)
    e = _row_err(a, ref)
    print(f"\nnarrow: twins {ia[4]}, splits {ia[5]}; vs ref {e:.3e}")
    assert ia[5] > 0, ia
    assert torch.isfinite(a).all() and float(a.min()) >= 0.0
    assert e <= TOL


def test_twin_tilted_gaussians():
    """Needles (one log-scale +1.5, the other two -1, random rotations): adjacent rays' closest-approach bins
    differ by tens of bins, so the unions are much longer than either segment."""
    from nlosgr import _lib
    def needle(m):
        m._scaling[:, 0] += 1.5
        m._scaling[:, 1:] -= 1.0
    P, geo, cfg = _setup(_scene(), edit=needle)
    ref = _chunk_sum(P, geo, cfg)
    a, ia = _fx(P, geo, cfg)
    _, istat = _fx(P, geo, cfg, _lib.FLAG_FX_TWIN_STATS)
    e = _row_err(a, ref)
    print(f"\ntilted: twins {ia[4]}, splits {ia[5]}, largest union {istat[6]} bins; vs ref {e:.3e}")
    assert ia[4] > 0, ia
    assert e <= TOL


@pytest.mark.parametrize("case", ["first_bin", "last_bin"])
def test_twin_clipped_segments(case):
    """The radial grid cuts through the hidden volume (y in [0.25, 0.75]): its first bin at r = 0.5, or its
    last bin at r = 0.53 (96 bins of 5e-3 from r = 0.05), so unions are clipped at bin 0 / bin nr - 1.  (The bin
    width stays 5e-3.  On 2e-3 bins every ray of every Gaussian reaches every bin, 64k terms of a few units
    each, and the FX drains' rounding of every term to a unit shows: measured there against this reference,
    single-segment drain 7.0e-5, twin drain 2.8e-5, the reference itself 2.6e-6 between chunks of 250 and 25.)"""
    scene = _scene(start=100) if case == "first_bin" else _scene(T=96, start=10, deltaT=5e-3)
    P, geo, cfg = _setup(scene)
    ref = _chunk_sum(P, geo, cfg)
    a, ia = _fx(P, geo, cfg)
    edge = 0 if case == "first_bin" else geo.nr - 1
    e = _row_err(a, ref)
    print(f"\nclipped {case}: r [{float(geo.r[0]):.3f}, {float(geo.r[-1]):.3f}], twins {ia[4]}, splits {ia[5]}; "
          f"edge bin / row max {float((ref[:, edge] / ref.max(1).values).min()):.3f}; vs ref {e:.3e}")
    assert ia[4] > 0, ia
    assert float(ref[:, edge].min()) > 0.0, "the edge bin is empty: nothing was clipped"
    assert e <= TOL


def test_twin_none_possible_equals_single():
    """Gaussians of sigma 1.5e-4: 5.7 sigma is 1.7e-3 across, under half the narrowest spacing of adjacent
    rays where they meet the volume (angular steps of 0.027 rad and more at r >= 0.25 with sin(theta) >= 0.6:
    4e-3), so no two adjacent cells pass: no twin is formed and the output equals the single-segment drain's
    bit for bit."""
    from nlosgr import _lib
    def tiny(m):
        m._scaling[:] = math.log(1.5e-4)
    P, geo, cfg = _setup(_scene(), edit=tiny)
    a, ia = _fx(P, geo, cfg)
    b, ib = _fx(P, geo, cfg, _lib.FLAG_FX_NOTWIN)
    print(f"\nno twin: twins {ia[4]}, splits {ia[5]}, sum {float(a.sum()):.4e}")
    assert ia[4] == 0 and ia[5] == 0, ia
    assert float(a.sum()) > 0.0
    assert torch.equal(a, b)


def test_fx_info_zero_after_float_drain():
    """A FLAG_FLOAT_DRAIN forward on a workspace that an FX forward used before leaves fx_info all zeros."""
    from nlosgr import _lib
    from nlosgr.render import fx_info, render_forward, workspace_for
    P, geo, cfg = _setup(_scene())
    ws = workspace_for(*P, geo, cfg)
    render_forward(*P, geo, cfg, workspace=ws)
    assert any(fx_info(*P, geo, cfg, ws)), "the FX forward left no info"
    fcfg = replace(cfg, flags=_lib.FLAG_FLOAT_DRAIN)
    render_forward(*P, geo, fcfg, workspace=ws)
    assert fx_info(*P, geo, fcfg, ws) == (0, 0, 0, 0, 0, 0, 0)
