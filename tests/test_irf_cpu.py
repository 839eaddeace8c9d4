"""Temporal instrument response on the CPU (no GPU): gaussian_irf's shape, IRF's validation, convolve_time's
conv1d fallback against the float64 oracle (tests/irf_oracle.py), its autograd and adjoint, the capture
file's optional IRF fields and the data_kwargs["irf"] hook of nlos_helpers.compute_loss."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import irf_oracle as IO


def _fwhm(w):
    """Full width at half maximum of sampled taps, the crossings interpolated linearly."""
    w = np.asarray(w, dtype=np.float64)
    p = int(np.argmax(w))
    half = w[p] / 2
    lo = p
    while lo > 0 and w[lo] > half:
        lo -= 1
    hi = p
    while hi < w.size - 1 and w[hi] > half:
        hi += 1
    left = lo + (half - w[lo]) / (w[lo + 1] - w[lo])
    right = hi - (half - w[hi]) / (w[hi - 1] - w[hi])
    return right - left


@pytest.mark.parametrize("fwhm", [2.5, 6.0, 40.0])
def test_gaussian_irf_shape(fwhm):
    from nlosgr.irf import gaussian_irf
    irf = gaussian_irf(fwhm)
    w = irf.taps.double().numpy()
    assert abs(w.sum() - 1.0) <= 1e-6
    assert irf.center == int(np.argmax(w)) and irf.background == 0.0
    assert abs(_fwhm(w) - fwhm) <= 1.0
    np.testing.assert_allclose(w, w[::-1], rtol=0, atol=1e-9)      # symmetric without a tail


def test_gaussian_irf_tail_leans_late():
    from nlosgr.irf import gaussian_irf
    irf = gaussian_irf(6.0, tail_bins=3.0, background=0.25)
    w = irf.taps.double().numpy()
    c = irf.center
    assert abs(w.sum() - 1.0) <= 1e-6 and c == int(np.argmax(w)) and irf.background == 0.25
    assert w[c + 1:].sum() > w[:c].sum()                         # more mass after the peak than before it
    k = np.arange(w.size) - c
    assert (w * k).sum() > 0.5                                   # and the mean delay is late
    with pytest.raises(ValueError):
        gaussian_irf(400.0)                                      # needs more than 512 taps


def test_irf_validation():
    from nlosgr.irf import IRF
    with pytest.raises(ValueError):
        IRF(np.zeros(0))
    with pytest.raises(ValueError):
        IRF(np.ones(513))
    with pytest.raises(ValueError):
        IRF(np.ones(4), center=4)
    with pytest.raises(ValueError):
        IRF(np.ones(4), center=-1)
    with pytest.raises(ValueError):
        IRF(np.ones((2, 2)))
    a = IRF(np.ones(512), center=511, background=0.5)
    assert len(a) == 512 and a.center == 511 and a.background == 0.5
    b = IRF(torch.tensor([0.5, 2.0, -0.5]))
    assert b.center == 1 and b.taps.dtype == torch.float32
    n = b.normalized()
    assert abs(n.taps.sum().item() - 1.0) <= 1e-6 and n.center == 1
    assert b.to("cpu") is b


def _case(nr, L, c, rows=3, seed=0):
    g = np.random.default_rng(seed + 7 * nr + L)
    h = (g.random((rows, nr)) * (g.random((rows, nr)) > 0.5)).astype(np.float32)
    w = g.standard_normal(L).astype(np.float32)
    return h, w


@pytest.mark.parametrize("nr,L,c", [(1, 1, 0), (7, 33, 16), (65, 255, 0), (100, 64, 63)])
def test_convolve_time_cpu_matches_oracle(nr, L, c):
    from nlosgr.irf import IRF, adjoint_time, convolve_time
    h, w = _case(nr, L, c)
    irf = IRF(w, c, background=0.125)
    x = torch.from_numpy(h).double()
    y = convolve_time(x, irf).numpy()
    ref = IO.apply64(h, w, c, 0.125)
    bound, _ = IO.apply_bound(h, w, c, 0.125)
    assert np.all(np.abs(y - ref) <= 1e-12 * bound / IO.U)      # float64 against float64: 2^-53-level slack
    z = adjoint_time(x, irf).numpy()
    ref = IO.adjoint64(h, w, c)
    bound, _ = IO.adjoint_bound(h, w, c)
    assert np.all(np.abs(z - ref) <= 1e-12 * bound / IO.U)
    # float32 fallback: the running-error bound of the fp32 sum
    y32 = convolve_time(torch.from_numpy(h), irf).numpy()
    bound, _ = IO.apply_bound(h, w, c, 0.125)
    assert np.all(np.abs(y32 - IO.apply64(h, w, c, 0.125)) <= bound)
    # a 1-D histogram is one row
    y1 = convolve_time(x[0], irf)
    assert y1.shape == (nr,) and torch.equal(y1, convolve_time(x, irf)[0])


def test_emulated_fp32_chain_is_within_the_bound():
    """The kernels' arithmetic (sequential fp32 fma chain) restated on the CPU stays inside the bound the
    GPU tests use (-s prints the worst share of it)."""
    for nr, L, c in [(7, 33, 16), (65, 255, 0), (100, 64, 63)]:
        h, w = _case(nr, L, c)
        y = IO.emulate_apply32(h, w, c, 0.01)
        bound, A = IO.apply_bound(h, w, c, 0.01)
        err = np.abs(y.astype(np.float64) - IO.apply64(h, w, c, 0.01))
        print(f"emulated apply nr={nr} L={L} c={c}: worst err/bound {float((err[A > 0] / bound[A > 0]).max()):.3f}")
        assert np.all(err <= bound)


def test_convolve_time_gradcheck_and_adjoint():
    from nlosgr.irf import IRF, adjoint_time, convolve_time
    g = torch.Generator().manual_seed(0)
    irf = IRF(torch.randn(4, generator=g), center=1, background=0.3)
    x = torch.randn(2, 9, generator=g, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: convolve_time(t, irf), (x,))
    for nr, L, c in [(9, 4, 1), (65, 255, 0), (100, 64, 63), (7, 33, 16)]:
        irf = IRF(torch.randn(L, generator=g), center=c)            # no background: the linear part
        x = torch.randn(3, nr, generator=g, dtype=torch.float64)
        z = torch.randn(3, nr, generator=g, dtype=torch.float64)
        lhs = (convolve_time(x, irf) * z).sum().item()
        rhs = (x * adjoint_time(z, irf)).sum().item()
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def _capture(T=40, H=3, W=4, seed=0):
    g = np.random.default_rng(seed)
    data = g.random((T, H, W)).astype(np.float32)
    xs = np.linspace(-0.5, 0.5, W)
    zs = np.linspace(-0.5, 0.5, H)
    pos = np.stack([np.repeat(xs[None, :], H, 0).reshape(-1), np.zeros(H * W), np.repeat(zs[:, None], W, 1).reshape(-1)])
    return data, pos.astype(np.float32)


def test_capture_file_irf_round_trip(tmp_path):
    from nlosgr.data import load_irf, load_zaragoza, make_data_kwargs, save_zaragoza
    from nlosgr.irf import gaussian_irf
    data, pos = _capture()
    irf = gaussian_irf(6.0, tail_bins=3.0, background=0.02)
    f = tmp_path / "cap_irf.mat"
    save_zaragoza(str(f), data, pos, (0.0, 0.5, 0.0), 0.5, 0.01, 1.0, irf=irf)
    back = load_irf(str(f))
    assert torch.equal(back.taps, irf.taps) and back.center == irf.center and back.background == irf.background
    out = load_zaragoza(str(f))
    assert len(out) == 9
    np.testing.assert_array_equal(out[0], data)
    torch.manual_seed(0)
    dk, *_ = make_data_kwargs(str(f), "cpu")
    assert torch.equal(dk["irf"].taps, irf.taps) and dk["irf"].center == irf.center
    # a file without the fields: None, the same 9-tuple, no new key
    f2 = tmp_path / "cap.mat"
    save_zaragoza(str(f2), data, pos, (0.0, 0.5, 0.0), 0.5, 0.01, 1.0)
    assert load_irf(str(f2)) is None
    out2 = load_zaragoza(str(f2))
    assert len(out2) == 9
    for a, b in zip(out, out2):
        np.testing.assert_array_equal(a, b)
    torch.manual_seed(0)
    dk2, *_ = make_data_kwargs(str(f2), "cpu")
    assert "irf" not in dk2 and set(dk2) == set(dk) - {"irf"}


def test_compute_loss_irf_hook(monkeypatch):
    """compute_loss passes the prediction through data_kwargs["irf"] before the criterion: the identity IRF
    changes nothing, a real one gives the MSE of the convolved prediction, and gradients reach the render.
    (The render itself needs a GPU: it is replaced by a fixed differentiable prediction here.)"""
    from nlosgr import nlos_helpers as NH
    from nlosgr.geometry import volume_box_point
    from nlosgr.irf import IRF, gaussian_irf
    T, start = 24, 3
    g = torch.Generator().manual_seed(5)
    base = torch.rand(T, generator=g)
    scale = torch.ones((), requires_grad=True)

    def fake_render(args, model, data_kwargs, input_points, cam, I1, I2, num_r, dth, dph):
        assert num_r == T
        return None, base * scale
    monkeypatch.setattr(NH, "gaussian_transient_rendering", fake_render)
    args = SimpleNamespace(num_sampling_points=2, start=start, end=start + T, occlusion=False, scaling_modifier=1.0,
                           gt_times=100)
    vpos = torch.tensor([0.0, 0.5, 0.0])
    dk = {"nlos_data": torch.rand(start + T + 2, 1, 2, generator=g) * 1e-2,
          "camera_grid_positions": torch.tensor([[0.1, 0.0, -0.1], [-0.2, 0.0, 0.15]]).t().contiguous(),
          "volume_position": vpos, "volume_box_point": volume_box_point(vpos, 0.5), "deltaT": 2.0 ** -5, "c": 1.0}
    ok = {"m": 0, "N": 2, "n": 1, "criterion": torch.nn.MSELoss(reduction="mean")}
    loss0, eq0 = NH.compute_loss(args, None, dk, ok)
    loss1, eq1 = NH.compute_loss(args, None, dict(dk, irf=IRF([1.0], 0, 0.0)), ok)
    assert loss1.item() == loss0.item() and eq1.item() == eq0.item()
    irf = gaussian_irf(4.0, tail_bins=2.0, background=0.05)
    loss2, _ = NH.compute_loss(args, None, dict(dk, irf=irf), ok)
    target = dk["nlos_data"][start:start + T, 0, 1].double().numpy() * 100
    y = IO.apply64(base.numpy()[None], irf.taps.numpy(), irf.center, irf.background)[0]
    ref = ((y - target) ** 2).mean()
    assert abs(loss2.item() - ref) <= 1e-5 * ref
    (gs,) = torch.autograd.grad(loss2, scale)
    ref_g = (2.0 / T) * ((y - target) * (y - irf.background)).sum()    # dy/dscale = y - b at scale 1
    assert abs(gs.item() - ref_g) <= 1e-4 * abs(ref_g)
