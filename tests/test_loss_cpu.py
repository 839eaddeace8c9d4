"""Photon-count likelihood on the CPU (no GPU): the float64 oracle's identities (tests/loss_oracle.py), the plain-torch
PoissonDeviance against it (values, gradcheck, as the criterion of nlos_helpers.compute_loss behind the IRF hook),
the host validation of nlosgr_loss_irf through ctypes (nothing is launched) and simulate_capture's CPU path."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import irf_oracle as IO
import loss_oracle as LO


def _case(rows=3, nr=40, L=9, seed=0, b=0.01):
    g = np.random.default_rng(seed)
    k = np.arange(L, dtype=np.float64)
    w = np.exp(-0.5 * ((k - (L - 1) / 2) / (L / 8 + 0.5)) ** 2)
    w = (w / w.sum()).astype(np.float32)
    h = (20.0 * g.random((rows, nr)) * (g.random((rows, nr)) > 0.7)).astype(np.float32)
    lam = IO.apply64(h, w, L // 2, np.float32(b))
    target = g.poisson(lam).astype(np.float32)
    return h, w, L // 2, np.float32(b), target


@pytest.mark.parametrize("eps", [1.0, 1e-3])
def test_oracle_deviance_identities(eps):
    h, w, c, b, target = _case()
    lam = IO.apply64(h, w, c, b)
    yp, rho, dev, q, ycount = LO.elements64(lam, target, 1.0, eps)
    assert np.all(dev >= 0.0) and (target == 0).any() and np.isfinite(dev).all()
    ref = LO.deviance64(rho, yp)                                  # the textbook form of the same quantity
    assert np.all(np.abs(dev - ref) <= 1e-12 * (1.0 + np.abs(yp * np.log(yp / rho)) + yp + rho))
    # rho = y' (a perfect fit): exactly 0, and a zero gradient factor
    yp0, rho0, dev0, q0, _ = LO.elements64(np.maximum(target.astype(np.float64), 0.0), target, 1.0, eps)
    assert np.array_equal(yp0, rho0) and not dev0.any() and not q0.any()
    # negative targets count as no photons; a negative rate is clamped: no NaN, no gradient there
    yp1, rho1, dev1, q1, yc1 = LO.elements64(-np.abs(lam) - 1.0, -np.abs(target) - 1.0, 1.0, eps)
    assert np.isfinite(dev1).all() and not dev1.any() and not q1.any() and not yc1.any()
    loss4, grad, bound, _ = LO.poisson_irf64(h, target, 1.0, w, c, b, eps, 1.0)
    assert loss4[0] == loss4[2] / h.size and loss4[1] == loss4[2] / loss4[3] and loss4[3] == target.sum()
    assert np.all(bound > 0) and np.isfinite(grad).all()


@pytest.mark.parametrize("eps", [1.0, 1e-3])
def test_oracle_gradient_is_the_central_difference(eps):
    rows, nr = 2, 12
    h, w, c, b, target = _case(rows, nr, L=5, seed=3)
    h = h + np.float32(0.5)                                        # lambda > 0 everywhere: no kink inside the step
    gs = 0.75
    _, grad, _, _ = LO.poisson_irf64(h, target, 2.0, w, c, b, eps, gs)
    step = 1e-5
    for p in range(rows):
        for t in range(nr):
            hp, hm = h.astype(np.float64), h.astype(np.float64)
            hp[p, t] += step
            hm[p, t] -= step
            fd = (LO.loss64(hp, target, 2.0, w, c, b, eps, gs) - LO.loss64(hm, target, 2.0, w, c, b, eps, gs)) / (2 * step)
            assert abs(fd - grad[p, t]) <= 1e-6 * max(abs(grad[p, t]), np.abs(grad).max() * 1e-3), (p, t)


def test_emulated_fp32_sequence_is_within_the_bound():
    """The kernel's element sequence restated in numpy fp32 (irf_oracle.emulate_apply32 for both convolutions) stays
    inside the bound the GPU test uses (-s prints the worst share of it)."""
    for eps in (1.0, 1e-3):
        for nr, L in [(7, 33), (65, 255), (100, 64)]:
            h, w, c, b, target = _case(3, nr, L, seed=nr)
            gs = 0.5
            loss4, grad, bound, _ = LO.poisson_irf64(h, target, 1.0, w, c, b, eps, gs)
            lam32 = IO.emulate_apply32(h, w, c, b)
            z, dev = LO.emulate_poisson32(lam32, target, 1.0, eps, np.float32(gs * 2.0 / h.size))
            g32 = IO.emulate_apply32(z, w[::-1].copy(), L - 1 - c)   # the adjoint: reversed taps, mirrored centre
            err = np.abs(g32.astype(np.float64) - grad)
            rel = abs(float(dev.astype(np.float64).sum()) - loss4[2]) / loss4[2]
            print(f"emulated poisson eps={eps} nr={nr} L={L}: gradient err/bound {float((err / bound).max()):.3f}  "
                  f"sum dev rel {rel:.2e}")
            assert np.all(err <= bound) and rel <= 1e-5


@pytest.mark.parametrize("eps", [1.0, 1e-3])
def test_poisson_deviance_matches_oracle_and_gradchecks(eps):
    from nlosgr.loss import PoissonDeviance
    h, w, c, b, target = _case()
    lam = IO.apply64(h, w, c, b)
    _, _, dev, q, _ = LO.elements64(lam, target, 1.0, eps)
    crit = PoissonDeviance(float(np.float32(eps)))                # (the oracle reads eps as the kernel does, in fp32)
    pred = torch.from_numpy(lam).requires_grad_(True)
    out = crit(pred, torch.from_numpy(target).double())
    assert abs(out.item() - dev.mean()) <= 1e-12 * dev.mean()
    (g,) = torch.autograd.grad(out, pred)
    ref = 2.0 * q / lam.size
    assert np.all(np.abs(g.numpy() - ref) <= 1e-12 * np.abs(ref).max())
    gen = torch.Generator().manual_seed(1)
    x = (torch.rand(2, 7, generator=gen, dtype=torch.float64) * 5 + 0.1).requires_grad_(True)
    t = torch.poisson(torch.rand(2, 7, generator=gen, dtype=torch.float64) * 5, generator=gen)
    assert torch.autograd.gradcheck(lambda p: crit(p, t), (x,))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            PoissonDeviance(bad)


def test_poisson_deviance_is_a_compute_loss_criterion(monkeypatch):
    """PoissonDeviance as optim_kwargs["criterion"]: compute_loss passes the prediction through data_kwargs["irf"]
    first, so the criterion sees the model rate; gradients reach the render.  (The render itself needs a GPU: it is
    replaced by a fixed differentiable prediction, as in test_compute_loss_irf_hook.)"""
    from nlosgr import nlos_helpers as NH
    from nlosgr.geometry import volume_box_point
    from nlosgr.irf import gaussian_irf
    from nlosgr.loss import PoissonDeviance
    T, start = 24, 3
    g = torch.Generator().manual_seed(5)
    base = torch.rand(T, generator=g) * 8
    scale = torch.ones((), requires_grad=True)

    def fake_render(args, model, data_kwargs, input_points, cam, I1, I2, num_r, dth, dph):
        assert num_r == T
        return None, base * scale
    monkeypatch.setattr(NH, "gaussian_transient_rendering", fake_render)
    args = SimpleNamespace(num_sampling_points=2, start=start, end=start + T, occlusion=False, scaling_modifier=1.0,
                           gt_times=100)
    vpos = torch.tensor([0.0, 0.5, 0.0])
    dk = {"nlos_data": torch.poisson(torch.rand(start + T + 2, 1, 2, generator=g) * 6, generator=g) * 1e-2,
          "camera_grid_positions": torch.tensor([[0.1, 0.0, -0.1], [-0.2, 0.0, 0.15]]).t().contiguous(),
          "volume_position": vpos, "volume_box_point": volume_box_point(vpos, 0.5), "deltaT": 2.0 ** -5, "c": 1.0}
    irf = gaussian_irf(4.0, tail_bins=2.0, background=0.05)
    eps = 0.5
    ok = {"m": 0, "N": 2, "n": 1, "criterion": PoissonDeviance(eps)}
    loss, _ = NH.compute_loss(args, None, dict(dk, irf=irf), ok)
    target = dk["nlos_data"][start:start + T, 0, 1].numpy()
    w, c, b = irf.taps.numpy(), irf.center, np.float32(irf.background)
    loss4, _, _, lam = LO.poisson_irf64(base.numpy()[None], target[None], 100.0, w, c, b, eps, 1.0)
    assert abs(loss.item() - loss4[0]) <= 1e-5 * loss4[0]
    (gs,) = torch.autograd.grad(loss, scale)
    _, _, _, q, _ = LO.elements64(lam, target[None], 100.0, eps)
    ref_g = (2.0 / T) * (q * (lam - float(b))).sum()              # dlambda/dscale = lambda - b at scale 1
    assert abs(gs.item() - ref_g) <= 1e-4 * abs(ref_g)


def test_loss_irf_host_validation():
    """nlosgr_loss_irf validates on the host, the loss first: every call here returns before anything is launched."""
    from nlosgr import _lib
    lib = _lib.load()
    assert ctypes.sizeof(_lib.Loss) == 8
    assert lib.nlosgr_abi_version() == 13 and _lib.ABI_VERSION == 13
    for rows in (0, 1, 1000, 16384):
        assert lib.nlosgr_loss_irf_workspace_bytes(rows) == lib.nlosgr_mse_irf_workspace_bytes(rows)
    fake = ctypes.c_void_p(4096)                                   # validation only checks that pointers are set
    irf = ctypes.byref(_lib.Irf(8, 0, fake, 0.0))

    def call(loss, i=irf, rows=2, nr=16, ws=fake):
        return lib.nlosgr_loss_irf(fake, fake, 1.0, rows, nr, i, loss, 1.0, fake, ws, fake, None)

    def spec(kind, floor=1.0):
        return ctypes.byref(_lib.Loss(kind, floor))
    assert call(None) == 1 and b"null loss" in lib.nlosgr_last_error()
    for kind in (2, -1, 7):
        assert call(spec(kind)) == 1 and b"kind" in lib.nlosgr_last_error()
    bad = (0.0, -1.0, float("nan"), float("inf"), -float("inf"))
    for floor in bad:
        assert call(spec(_lib.LOSS_POISSON, floor)) == 1 and b"rate_floor" in lib.nlosgr_last_error()
    # a valid loss passes on to the checks nlosgr_mse_irf has (shown by their messages); MSE ignores rate_floor
    for s in [spec(_lib.LOSS_POISSON, 1.0), spec(_lib.LOSS_POISSON, 1e-30)] + [spec(_lib.LOSS_MSE, f) for f in bad]:
        assert call(s, ws=None) == 1 and b"workspace" in lib.nlosgr_last_error()
        assert call(s, nr=0) == 1 and b"nr" in lib.nlosgr_last_error()
        assert call(s, rows=-1) == 1 and b"rows" in lib.nlosgr_last_error()
        assert call(s, nr=_lib.IRF_MAX_NR + 1) == 3 and b"nr" in lib.nlosgr_last_error()
        assert call(s, i=None) == 1 and b"irf" in lib.nlosgr_last_error()
        assert call(s, i=ctypes.byref(_lib.Irf(513, 0, fake, 0.0))) == 1 and b"ntaps" in lib.nlosgr_last_error()


def test_loss_python_argument_checks():
    from nlosgr.loss import loss
    from nlosgr.train import TrainStep
    x = torch.zeros(2, 4)
    with pytest.raises(ValueError):
        loss(x, x, kind="huber")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            loss(x, x, kind="poisson", rate_floor=bad)
    with pytest.raises(ValueError):
        TrainStep(None, None, None, x, loss="huber")


def test_simulate_capture_cpu():
    from nlosgr.irf import gaussian_irf
    from nlosgr.loss import simulate_capture
    gen = torch.Generator().manual_seed(7)
    hist = torch.rand(6, 50, generator=gen) * (torch.rand(6, 50, generator=gen) > 0.6) * 30
    irf = gaussian_irf(5.0, tail_bins=2.0, background=0.2)
    a, sa = simulate_capture(hist, irf, generator=torch.Generator().manual_seed(11))
    b, sb = simulate_capture(hist, irf, generator=torch.Generator().manual_seed(11))
    assert torch.equal(a, b) and sa == sb == 1.0
    assert a.dtype == torch.float32 and a.shape == hist.shape
    assert torch.all(a >= 0) and torch.equal(a, a.round())
    c, _ = simulate_capture(hist, irf, generator=torch.Generator().manual_seed(12))
    assert not torch.equal(a, c)
    # without an IRF the rate is the render itself: a zero rate gives zero counts, negative values count as zero
    z, _ = simulate_capture(torch.zeros(3, 9))
    assert not z.any()
    n, _ = simulate_capture(-hist)
    assert not n.any()
    d, _ = simulate_capture(hist, generator=torch.Generator().manual_seed(1))
    assert not d[hist == 0].any() and d.sum() > 0
    # photons: the rate sums to N, the total count is a Poisson draw of mean N
    from nlosgr.irf import convolve_time
    N = 250000.0
    counts, scale = simulate_capture(hist, irf, photons=N, generator=torch.Generator().manual_seed(3))
    rate = convolve_time(hist, irf).clamp_min(0).double() * scale
    assert abs(rate.sum().item() - N) <= 1e-5 * N
    assert abs(counts.double().sum().item() - N) <= 6.0 * math.sqrt(N)
    one, _ = simulate_capture(hist[0], irf, photons=100.0, generator=torch.Generator().manual_seed(3))
    assert one.shape == (50,)
