"""Refills of the twin drain of the no-occlusion fixed-point (FX) forward (csrc/nlosgr_volume_fwd.hip, fwd_body).

Once a chunk's enumeration is exhausted the twin drain refills only when the idle lanes can take the whole queue
(or the steady threshold), its deal moves a packed state word and recomputes the peak sum in the headroom re-arm,
and it places no segment early.  None of this may change which (pair, cell) groups are drained, and a wrong
refill rule is a hang, so every shape here must end and must give the histogram of the one-ray-per-lane drain
(FLAG_FX_NOTWIN) and of the reference: the float64 sum of fp32 FLAG_FLOAT_DRAIN sub-histograms, within 2e-5 of
each row's maximum (the comparison and tolerance of tests/test_gpu_fx_runs.py), bitwise equal run to run.
3 x 3 wall points, 256 bins, ns 16, 5.7 sigma, cuda preset unless said otherwise.  Figures are printed (pytest -s).

The sub-histograms hold 250 Gaussians each, as in tests/test_gpu_fx_runs.py, except for the piles: there every
Gaussian adds to the same bins, and an fp32 bin that sums n equal terms carries an error of about sqrt(n) 6e-8
(n = 250 Gaussians x 256 rays: 1.5e-5, the tolerance itself), so the piles use 16 Gaussians per sub-histogram
(n = 4096: 4e-6).
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
C0 = 0.28209479177387814


def _params(m):
    from nlosgr import features_flat
    return [m._mu.detach(), m._scaling.detach(), m._rotation.detach(), m._opacity.detach(),
            features_flat(m).detach().contiguous()]


def _chunk_sum(P, geo, cfg, chunk):
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


def _scene(T=256, ns=16, H=3, W=3, **kw):
    from nlosgr.volume import Scene
    return Scene(H=H, W=W, T=T, ns=ns, **kw)


def _setup(scene, ng, edit=None, seed=21):
    from nlosgr import GaussianParams
    from nlosgr.volume import make_config
    dev = torch.device("cuda:0")
    m = GaussianParams.synthetic(ng, 3, preset="cuda", device=dev, seed=seed)
    if edit is not None:
        with torch.no_grad():
            edit(m)
    return _params(m), scene.geometry(dev, "cuda", "noocl"), make_config(m, scene, "cuda", "noocl", cutoff=CUT)


def _check(name, P, geo, cfg, chunk=250):
    """The default drain against the reference and the one-ray drain, and against itself; returns its info."""
    from nlosgr import _lib
    ref = _chunk_sum(P, geo, cfg, chunk)
    a, ia = _fx(P, geo, cfg)
    a2, ia2 = _fx(P, geo, cfg)
    b, ib = _fx(P, geo, cfg, _lib.FLAG_FX_NOTWIN)
    ea, eb, eab = _row_err(a, ref), _row_err(b, ref), _row_err(a, b.double())
    print(f"\n{name}: groups {ia[4]}, splits {ia[5]}, flushes {ia[2]}, bright {ia[3]}; default vs ref {ea:.3e}, "
          f"single vs ref {eb:.3e}, default vs single {eab:.3e} (of each row's max)")
    assert torch.isfinite(a).all() and float(a.min()) >= 0.0
    assert ib[4] == 0 and ib[5] == 0, ib
    assert ea <= TOL and eb <= TOL and eab <= TOL
    assert torch.equal(a, a2) and ia == ia2
    return a, ia


def test_1500_gaussians():
    """1500 Gaussians: the launch cuts them into 6 splits of 256 per wall point, one chunk for each of a
    workgroup's 4 waves; every chunk's tail crosses the min(threshold, queue) switch.  Twins are formed."""
    P, geo, cfg = _setup(_scene(), 1500)
    a, ia = _check("1500", P, geo, cfg)
    assert ia[4] > 0, ia
    assert float(a.sum()) > 0.0


def test_segments_carry_over_between_chunks():
    """2600 Gaussians: the launch has at most 8 splits, here of 384 Gaussians, so two waves of every workgroup
    drain a second chunk, which starts with the first chunk's segments still running in its lanes."""
    P, geo, cfg = _setup(_scene(), 2600)
    _, ia = _check("2600", P, geo, cfg)
    assert ia[4] > 0, ia


def test_seventy_gaussians():
    """70 Gaussians: one wave has a full chunk, the next a chunk of 6 live lanes, whose queue in the tail is far
    below the threshold."""
    P, geo, cfg = _setup(_scene(), 70)
    a, _ = _check("70", P, geo, cfg)
    assert float(a.sum()) > 0.0


def test_one_gaussian():
    """A single pair per wall point: its queue never reaches the threshold, and the drain ends."""
    P, geo, cfg = _setup(_scene(), 1)
    a, _ = _check("1", P, geo, cfg)
    assert float(a.sum()) > 0.0


def test_no_gaussians():
    """No Gaussian at all: the forward ends and the histogram is zero."""
    from nlosgr.render import render_forward
    P, geo, cfg = _setup(_scene(), 1)
    h, _ = render_forward(*[t[:0].contiguous() for t in P], geo, cfg)
    torch.cuda.synchronize()
    assert h.shape == (geo.nwall, geo.nr) and float(h.abs().max()) == 0.0


def _pile(ng, jitter, H=2, seed=5):
    """ng co-located, equally bright, wide Gaussians (the Gaussians of tests/test_gpu_fx.py's flush pile, which has 2 x 2 wall
    points): none is 'bright', and their sum drives a wave's LDS fields past 2^31 units."""
    from nlosgr import GaussianParams
    from nlosgr.volume import make_config
    dev = torch.device("cuda:0")
    scene = _scene(H=H, W=H)
    g = torch.Generator().manual_seed(seed)
    mu = torch.tensor(scene.volume_position).float().repeat(ng, 1)
    scaling = torch.full((ng, 3), float(np.log(0.06)))
    rotation = torch.randn(1, 4, generator=g).repeat(ng, 1)
    if jitter:
        mu = mu + 1e-3 * torch.randn(ng, 3, generator=g)
        scaling = scaling + 0.05 * torch.randn(ng, 3, generator=g)
        rotation = torch.randn(ng, 4, generator=g)
    opacity = torch.full((ng, 1), 4.0)
    fdc = torch.full((ng, 1, 1), (1.0 - 0.5) / C0)
    frest = torch.zeros(ng, 15, 1)
    m = GaussianParams(*(t.float().to(dev).contiguous() for t in (mu, scaling, rotation, opacity, fdc, frest)), 3, 3)
    return _params(m), scene.geometry(dev, "cuda", "noocl"), make_config(m, scene, "cuda", "noocl", cutoff=CUT)


def test_identical_gaussians():
    """64 identical, co-located Gaussians (one chunk of one wave): every queue entry of a row has the same first
    bin, so the deal has nothing to spread; the wave's 64 x 256 segments of equal peak pass the lanes' headroom
    many times over, so the re-arm reads the recomputed peak sums, and the fields are flushed."""
    P, geo, cfg = _pile(64, jitter=False, H=3)
    _, ia = _check("64 identical", P, geo, cfg, chunk=16)
    assert ia[2] > 0, "the LDS flush did not run"
    assert ia[3] == 0 and ia[4] > 0, ia


def test_flush_pile():
    """The flush pile of tests/test_gpu_fx.py at a third of its size (256 Gaussians, one per lane of a workgroup)."""
    P, geo, cfg = _pile(256, jitter=True)
    _, ia = _check("pile 256", P, geo, cfg, chunk=16)
    assert ia[2] > 0, "the LDS flush did not run"
    assert ia[3] == 0, ia


def test_thin_gaussians_requeue_in_the_tail():
    """One axis of every Gaussian 3e-4 long (tests/test_gpu_fx_runs.py): many twins are split at the merge guard
    and their second rays go back to the queue, also after the enumeration has ended, when the queue grows under
    a refill rule that looks at its length."""
    def thin(m):
        m._scaling[:, 1] = math.log(3e-4)
    P, geo, cfg = _setup(_scene(), 1500, edit=thin)
    _, ia = _check("thin axis", P, geo, cfg)
    assert ia[5] > 0, ia


def test_ns5():
    """ns 5: boxes narrower than a trip, short queues."""
    P, geo, cfg = _setup(_scene(ns=5), 1500)
    a, _ = _check("ns 5", P, geo, cfg)
    assert float(a.sum()) > 0.0


def test_41_bins_clipped_at_both_ends():
    """T = 41 bins of 5e-3 from r = 0.45 to 0.65, inside the hidden volume: unions start at bin 0 and end at bin
    nr - 1, and nr is odd."""
    P, geo, cfg = _setup(_scene(T=41, start=90, deltaT=5e-3), 1500)
    a, ia = _check("T 41", P, geo, cfg)
    assert geo.nr == 41 and ia[4] > 0
    assert float(a[:, 0].min()) > 0.0 and float(a[:, -1].min()) > 0.0, "nothing was clipped"
