"""Run-following pairs of the no-occlusion fixed-point (FX) forward (csrc/nlosgr_volume_fwd.hip, enumerate_runs;
csrc/nlosgr_enum.hpp, trip_plan).

The enumeration tests 4 cells of one row of a pair's box per trip and pairs passing cells along their run, so a
run of passing cells is no longer cut where a trip ends.  Which rays share a lane changes the result only within
the fixed-point rounding (one rounding per group) and the exact sub-cutoff tails inside unions, so these tests
pin the default drain against the one-ray-per-lane drain (FLAG_FX_NOTWIN) and the float64 sum of fp32
FLAG_FLOAT_DRAIN sub-histograms of 250 Gaussians each, at the tolerance of tests/test_gpu_fx.py and
tests/test_gpu_fx_twin.py (2e-5 of each row's maximum), and the number of groups it forms against a float64
replay of the enumeration on the CPU (nlosgr/enum_replay.py).  The small scene of tests/test_gpu_fx_twin.py: 1500
Gaussians, seed 21, 3 x 3 wall, 256 bins, ns 16, 5.7 sigma, cuda preset.  Figures are printed (pytest -s).
"""
import math
from dataclasses import replace

import numpy as np
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
    """(histogram, (E, E max, flushes, bright segments, groups, splits, ...)) of one FX forward."""
    from nlosgr.render import fx_info, render_forward, workspace_for
    c = replace(cfg, flags=flags)
    ws = workspace_for(*P, geo, c)
    h, _ = render_forward(*P, geo, c, workspace=ws)
    return h, fx_info(*P, geo, c, ws)


def _row_err(a, ref):
    """Largest error in units of each row's maximum (a row that is all zero in ref must be all zero in a)."""
    d, top = (a.double() - ref).abs().max(1).values, ref.abs().max(1).values
    assert bool((d[top == 0] == 0).all())
    return float((d[top > 0] / top[top > 0]).max()) if bool((top > 0).any()) else 0.0


def _model(seed=21, edit=None):
    from nlosgr import GaussianParams
    m = GaussianParams.synthetic(NG, 3, preset="cuda", device=torch.device("cuda:0"), seed=seed)
    if edit is not None:
        with torch.no_grad():
            edit(m)
    return m


def _setup(scene, edit=None):
    from nlosgr.volume import make_config
    m = _model(edit=edit)
    geo = scene.geometry(torch.device("cuda:0"), "cuda", "noocl")
    return m, _params(m), geo, make_config(m, scene, "cuda", "noocl", cutoff=CUT)


def _scene(T=256, ns=16, **kw):
    from nlosgr.volume import Scene
    return Scene(H=3, W=3, T=T, ns=ns, **kw)


def _replay(m, geo):
    """Per wall point: (box, ok) of nlosgr.enum_replay.wall_point_cells, pairs of w = sigma rho <= 0 dropped."""
    from nlosgr import enum_replay as E
    from oracle import torch_ref as R
    cpu = lambda t: t.detach().cpu()
    Pm = R.Params(cpu(m._mu), cpu(m._scaling), cpu(m._rotation), cpu(m._opacity), cpu(m._features_dc),
                  cpu(m._features_rest), int(m.active_sh_degree), requires_grad=False)
    mu = cpu(m._mu).numpy().astype(np.float64)
    A, smax = E.gaussian_frames(mu, cpu(m._scaling).numpy(), cpu(m._rotation).numpy())
    out = []
    for p in range(geo.nwall):
        box, ok, _, _ = E.wall_point_cells(geo, p, mu, A, smax, CUT)
        rho = R.albedo(Pm, cpu(geo.wall[p]).float(), preset="cuda")[:, 0].numpy()
        ok &= (rho > 0)[:, None, None]
        out.append((box, ok))
    return out


def test_default_vs_single_vs_reference():
    """The default drain, the one-ray-per-lane drain and the reference agree pairwise within 2e-5 of each row's
    maximum; groups were formed; two default runs are equal bit for bit, with the same counts."""
    from nlosgr import _lib
    _, P, geo, cfg = _setup(_scene())
    ref = _chunk_sum(P, geo, cfg)
    a, ia = _fx(P, geo, cfg)
    a2, ia2 = _fx(P, geo, cfg)
    b, ib = _fx(P, geo, cfg, _lib.FLAG_FX_NOTWIN)
    ea, eb, eab = _row_err(a, ref), _row_err(b, ref), _row_err(a, b.double())
    print(f"\nruns: groups {ia[4]}, splits {ia[5]}; default vs ref {ea:.3e}, single vs ref {eb:.3e}, "
          f"default vs single {eab:.3e} (of each row's max)")
    assert ia[4] > 0 and ib[4] == 0 and ib[5] == 0, (ia, ib)
    assert ea <= TOL and eb <= TOL and eab <= TOL
    assert torch.equal(a, a2) and ia == ia2


def test_pairing_quality():
    """Rays in groups against the float64 replay of the whole scene: more than the midpoint between the parent's
    trip pairing (3-cell row-major trips) and the per-row optimum, sum of floor(run / 2) pairs.  The margin of a
    quarter of the gap on each side covers cells whose quadric sign differs between fp32 and float64.
    Measured: 1 167 597 rays; trip replay 391 187 pairs, optimum 554 018, kernel 553 994 with 0 splits."""
    from nlosgr import enum_replay as E
    m, P, geo, cfg = _setup(_scene())
    _, ia = _fx(P, geo, cfg)
    assert ia[3] == 0, "a bright Gaussian would bypass the grouped drain"
    rays = trip = opt = run = 0
    for box, ok in _replay(m, geo):
        for g in np.nonzero(ok.any((1, 2)))[0]:
            i0, i1, j0, j1 = box[g]
            okb = ok[g, i0:i1 + 1, j0:j1 + 1]
            rays += int(okb.sum())
            trip += sum(l == 2 for _, _, l in E.groups_trip(okb)[0])
            run += sum(l == 2 for _, _, l in E.groups_run(okb, 2)[0])
            opt += E.row_optimum(okb) // 2
    print(f"\npairing: {rays} rays; pairs: trip replay {trip} ({2 * trip / rays:.3f} of rays), run replay {run} "
          f"({2 * run / rays:.3f}), per-row optimum {opt} ({2 * opt / rays:.3f}); kernel {ia[4]} "
          f"({2 * ia[4] / rays:.3f}), splits {ia[5]}")
    assert trip < opt
    assert ia[4] > 0.5 * (trip + opt), (ia, trip, opt)


def test_narrow_boxes_ns5():
    """ns 5: most boxes are narrower than a 4-cell trip, so every trip ends with its row."""
    from nlosgr import _lib
    _, P, geo, cfg = _setup(_scene(ns=5))
    a, ia = _fx(P, geo, cfg)
    b, _ = _fx(P, geo, cfg, _lib.FLAG_FX_NOTWIN)
    e = _row_err(a, b.double())
    print(f"\nns 5: groups {ia[4]}, splits {ia[5]}; default vs single {e:.3e}")
    assert float(b.sum()) > 0.0 and e <= TOL


def test_one_cell_wide_boxes_form_no_groups():
    """Gaussians of sigma 8e-4: the bounding sphere of 5.7 sigma spans 9.1e-3, under the narrowest spacing of
    adjacent rays in the volume (angular steps of 0.070 rad at r >= 0.25 with sin(theta) >= 0.6: 1.05e-2), so
    every box is at most one cell wide in phi (checked on the CPU replay, which finds 438 rays): no group can
    form, and the result agrees with the single drain's."""
    from nlosgr import _lib
    def tiny(m):
        m._scaling[:] = math.log(8e-4)
    m, P, geo, cfg = _setup(_scene(), edit=tiny)
    widest = max(int((box[:, 3] - box[:, 2] + 1).max()) for box, _ in _replay(m, geo))
    a, ia = _fx(P, geo, cfg)
    b, _ = _fx(P, geo, cfg, _lib.FLAG_FX_NOTWIN)
    e = _row_err(a, b.double())
    print(f"\none cell wide: widest box {widest}, groups {ia[4]}, splits {ia[5]}, sum {float(a.sum()):.4e}; "
          f"default vs single {e:.3e}")
    assert widest <= 1
    assert ia[4] == 0 and ia[5] == 0, ia
    assert float(a.sum()) > 0.0 and e <= TOL


def test_thin_axis_gaussians_split():
    """One axis of every Gaussian 3e-4 long (the split test of tests/test_gpu_fx_twin.py): groups are split at the
    merge guard, and the result stays finite, non-negative and within tolerance of the single drain."""
    from nlosgr import _lib
    def thin(m):
        m._scaling[:, 1] = math.log(3e-4)
    _, P, geo, cfg = _setup(_scene(), edit=thin)
    a, ia = _fx(P, geo, cfg)
    b, _ = _fx(P, geo, cfg, _lib.FLAG_FX_NOTWIN)
    e = _row_err(a, b.double())
    print(f"\nthin axis: groups {ia[4]}, splits {ia[5]}; default vs single {e:.3e}")
    assert ia[5] > 0, ia
    assert torch.isfinite(a).all() and float(a.min()) >= 0.0
    assert e <= TOL


def test_unions_clipped_at_both_ends():
    """T = 41 bins of 5e-3 from r = 0.45 to 0.65, inside the hidden volume (y in [0.25, 0.75]): unions are
    clipped at bin 0 and at bin nr - 1, and nr is odd."""
    from nlosgr import _lib
    _, P, geo, cfg = _setup(_scene(T=41, start=90, deltaT=5e-3))
    a, ia = _fx(P, geo, cfg)
    b, _ = _fx(P, geo, cfg, _lib.FLAG_FX_NOTWIN)
    e = _row_err(a, b.double())
    print(f"\nT 41: r [{float(geo.r[0]):.3f}, {float(geo.r[-1]):.3f}], groups {ia[4]}, splits {ia[5]}; "
          f"default vs single {e:.3e}")
    assert geo.nr == 41 and ia[4] > 0
    assert float(b[:, 0].min()) > 0.0 and float(b[:, -1].min()) > 0.0, "nothing was clipped"
    assert e <= TOL
