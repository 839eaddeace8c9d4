"""Pins the float64 volume reference (tests/volume_oracle.py) and its per-Gaussian metric.  No GPU is touched.

The reference is compared with the fp32 oracle (oracle.torch_ref.render_volume, itself pinned to the reference
implementation's golden vectors by test_oracle_golden.py) on the scene of test_gpu_parity.py::_volume_vs_oracle:
the forward within FWD_TOL of every row's maximum, every gradient within GAUSS_TOL per Gaussian in the metric of
volume_oracle (e_g <= tol s_g + b_g).  Both bounds are a few times the fp32 oracle's own rounding (measured:
3e-7 forward; per Gaussian <= 1.4e-6 on the broad scenes).  The narrow scene (log-scales - 3.5: Gaussians a
fraction of a bin wide, whose few samples sit on the steep flank of the pdf, where the fp32 rounding of a
sample's position is amplified by m^2 / 2 ~ 16) has bounds of its own, ten times the general ones: NARROW_TOL per
Gaussian (measured there <= 2.1e-5) and NARROW_FWD_TOL for the forward (measured 5.0e-6, the same amplification).
"""
import pytest
import torch

from conftest import ROOT  # noqa: F401

import volume_oracle as VO
from oracle import torch_ref as R

FWD_TOL = 5e-6
GAUSS_TOL = 1e-5
NARROW_TOL = 1e-4       # the narrow scene only (module docstring)
NARROW_FWD_TOL = 5e-5


def _fp32_oracle(model, k, preset, mode, cutoff, gout):
    P = VO.params_of_model(model)
    hist = R.render_volume(P, k["walls"], k["box"], k["Y"], k["ns"], k["start"], k["end"], k["c"], k["deltaT"],
                           preset=preset, mode=mode, mc=cutoff if cutoff > 0 else None)
    (hist * gout).sum().backward()
    return P, hist.detach(), [l.grad for l in P.leaves()]


def _compare(preset, mode, T, cutoff, tol, scale_shift=None, fwd_tol=FWD_TOL):
    model, geo, k = VO.parity_scene(preset, mode, T, scale_shift=scale_shift)
    gout = torch.randn(geo.nwall, geo.nr, generator=torch.Generator().manual_seed(5))
    P, hist, grads = _fp32_oracle(model, k, preset, mode, cutoff, gout)
    ref = VO.reference(P, geo, preset, mode, k["c"] * k["deltaT"], cutoff, gout)
    fw = VO.forward_worst(hist, ref)
    w = VO.worst(grads, ref)
    print(f"\n{preset} {mode} T={T} cutoff={cutoff} shift={scale_shift}: forward {fw:.2e}; per Gaussian "
          + ", ".join(f"{n} {v:.2e}" for n, v in w.items()))
    assert fw <= fwd_tol
    bad = VO.failures(grads, ref, tol)
    assert not bad, bad[:5]
    return ref


@pytest.mark.parametrize("preset", ["torch", "cuda"])
@pytest.mark.parametrize("mode", ["noocl", "netf"])
@pytest.mark.parametrize("T", [41, 97])
@pytest.mark.parametrize("cutoff", [5.7, 0.0])
def test_reference_matches_fp32_oracle(preset, mode, T, cutoff):
    """Odd row lengths, both presets and modes, 5.7 sigma and dense; on these broad Gaussians nothing is culled,
    so the bracket is exactly zero."""
    ref = _compare(preset, mode, T, cutoff, GAUSS_TOL)
    assert all(float(b.max()) == 0.0 for b in ref.bracket.values())
    assert all(float(s.min()) > 0.0 for s in ref.scale.values())


@pytest.mark.parametrize("mode", ["noocl", "netf"])
def test_reference_matches_fp32_oracle_narrow(mode):
    """The narrow scene under its own bound; its bracket is live and some Gaussians are reached by no sample."""
    ref = _compare("cuda", mode, 97, 5.7, NARROW_TOL, scale_shift=-3.5, fwd_tol=NARROW_FWD_TOL)
    s = ref.scale["mu"]
    assert int((s > 0).sum()) * 3 >= s.numel() and int((s == 0).sum()) > 0
    assert float(ref.bracket["mu"].max()) > 0.0


@pytest.mark.parametrize("name,g", [("mu", 7), ("opacity", 0), ("features_rest", 47)])
def test_planted_error_fails_exactly_that_gaussian(name, g):
    """1e-3 s_g added to one component of one Gaussian's row of one tensor fails that Gaussian of that tensor and
    nothing else at the tolerance of 2e-4; the reference's own gradients pass at zero tolerance; worst() reports
    the planted 1e-3."""
    model, geo, k = VO.parity_scene("cuda", "netf", 41)
    gout = torch.randn(geo.nwall, geo.nr, generator=torch.Generator().manual_seed(5))
    ref = VO.reference(VO.params_of_model(model), geo, "cuda", "netf", k["c"] * k["deltaT"], 5.7, gout)
    got = {n: t.clone() for n, t in ref.grads.items()}
    assert VO.failures(got, ref, 0.0) == []
    got[name][g, -1] += 1e-3 * ref.scale[name][g]
    bad = VO.failures(got, ref, 2e-4)
    assert [(b[0], b[1]) for b in bad] == [(name, g)], bad
    w = VO.worst(got, ref)
    assert abs(w[name] - 1e-3) < 1e-9 and all(v == 0.0 for n, v in w.items() if n != name)
    assert VO.failures(got, ref, 2e-3) == []


def test_unreached_gaussian_must_stay_within_bracket():
    """A Gaussian no sample reaches (s_g = 0) fails as soon as it is given a gradient beyond b_g."""
    model, geo, k = VO.parity_scene("cuda", "noocl", 97, scale_shift=-3.5)
    gout = torch.randn(geo.nwall, geo.nr, generator=torch.Generator().manual_seed(5))
    ref = VO.reference(VO.params_of_model(model), geo, "cuda", "noocl", k["c"] * k["deltaT"], 5.7, gout)
    dead = torch.nonzero(ref.scale["scaling"] == 0).flatten()
    assert dead.numel() > 0
    g = int(dead[0])
    got = {n: t.clone() for n, t in ref.grads.items()}
    assert VO.unreached_failures(got, ref) == []
    got["scaling"][g, 0] += 2.0 * float(ref.bracket["scaling"][g]) + 1e-12
    assert [(b[0], b[1]) for b in VO.unreached_failures(got, ref)] == [("scaling", g)]
    assert [(b[0], b[1]) for b in VO.failures(got, ref, 2e-4)] == [("scaling", g)]


def test_as_named_splits_the_flat_feature_gradient():
    ng, K = 5, 16
    five = [torch.randn(ng, 3), torch.randn(ng, 3), torch.randn(ng, 4), torch.randn(ng), torch.randn(ng, K)]
    d = VO.as_named(five)
    assert [tuple(d[n].shape) for n in VO.NAMES] == [(ng, 3), (ng, 3), (ng, 4), (ng, 1), (ng, 1), (ng, K - 1)]
    assert torch.equal(d["features_dc"][:, 0], five[4][:, 0].double())
    assert torch.equal(d["features_rest"], five[4][:, 1:].double())
