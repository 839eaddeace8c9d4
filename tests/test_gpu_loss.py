"""GPU checks of the photon-count likelihood of the fused loss (include/nlosgr.h nlosgr_loss_irf, csrc/nlosgr_irf.hip,
nlosgr.loss) against the float64 oracle of tests/loss_oracle.py:

  MSE kind          loss4 and gradient torch.equal to nlosgr_mse_irf on the IRF test's inputs (both tap kinds)
  POISSON gradient  per element |g - g64| <= bound, the derived bound of loss_oracle's docstring
  POISSON loss      all four floats of loss4 to 1e-5 relative of float64 (the project's number for the fused loss)
  clamp             signed taps with lambda well above 0: within the bound; rows with lambda < 0 throughout:
                    gradient rows exactly 0, deviance 2 [y' log(y'/eps) - y' + eps] to 1e-5
  no NaN            finite inputs, negative targets and rates included
  repeatability     two runs bitwise; rows [0,128) + [128,257) bitwise the whole call's gradient rows
  want_grad=False   the same loss4, no gradient; empty rows give zeros; no IRF == the identity IRF bitwise
  TrainStep(loss="poisson") == render -> conv1d -> PoissonDeviance -> torch.optim.Adam over 3 iterations (whole
                    wall, and the occlusion mode's wall-point batches)

Inputs: normalised Gaussian taps, h = 20 U(0,1) with 70 % exact zeros (bins at rho = b + eps occur), the target a
numpy Poisson draw from the float64 apply (zeros included), halved and given back by gt_times = 2.  Shapes: the
IRF test's seven, and the first row length of each further launch configuration (1025, 2049, 4097).  `-s` prints
the worst measured share of the bound per case.
"""
import ctypes
from dataclasses import replace

import numpy as np
import pytest
import torch

import irf_oracle as IO
import loss_oracle as LO

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 257]
IRF_SHAPES = [(1, 1, 0), (7, 33, 16), (63, 2, 1), (65, 255, 0), (1000, 255, 254), (1024, 512, 100), (8192, 129, 64)]
SHAPES = IRF_SHAPES + [(1025, 33, 10), (2049, 129, 64), (4097, 33, 0)]
BACKGROUNDS = [0.0, 0.01]
FLOORS = [1.0, 1e-3]
GT, GS = 2.0, 0.5
CASES = [(r, nr, L, c, b) for (nr, L, c) in SHAPES for r in ROWS for b in BACKGROUNDS]


def _gauss(L):
    k = np.arange(L, dtype=np.float64)
    w = np.exp(-0.5 * ((k - (L - 1) / 2) / (L / 8 + 0.5)) ** 2)
    return (w / w.sum()).astype(np.float32)


def _counts(g, lam):
    """A Poisson draw of the (non-negative part of the) rate, halved: gt_times = 2 gives the counts back exactly."""
    return (g.poisson(np.maximum(lam, 0.0)) / GT).astype(np.float32)


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"r{p[0]}-nr{p[1]}-L{p[2]}-c{p[3]}-b{p[4]}")
def case(request):
    """Inputs, the float64 apply and its A of one case, shared by both rate floors."""
    rows, nr, L, c, b = request.param
    g = np.random.default_rng(1000 * rows + nr + L)
    w = _gauss(L)
    keep = (g.random((rows, nr)) > 0.7) if nr > 1 else np.ones((rows, nr), dtype=bool)   # (1, 1, 0): sum dev != 0
    h = (20.0 * g.random((rows, nr)) * keep).astype(np.float32)
    b = np.float32(b)
    lam = IO.apply64(h, w, c, b)
    _, A = IO.apply_bound(h, w, c, b)
    return dict(rows=rows, nr=nr, L=L, c=c, b=b, w=w, h=h, lam=lam, A=A, target=_counts(g, lam))


def _irf(w, c, b=0.0):
    from nlosgr.irf import IRF
    return IRF(torch.from_numpy(np.asarray(w, dtype=np.float32)), c, float(b)).to("cuda:0")


def _share(err, bound):
    m = bound > 0
    return float((err[m] / bound[m]).max()) if m.any() else 0.0


def _close4(loss4, ref, tol=1e-5):
    return np.all(np.abs(loss4.double().cpu().numpy() - ref) <= tol * np.abs(ref))


def _poisson(h, target, irf, eps, **kw):
    from nlosgr.loss import loss
    return loss(torch.from_numpy(h).cuda(), torch.from_numpy(target).cuda(), GT, grad_scale=GS, raw=True, irf=irf,
                kind="poisson", rate_floor=eps, **kw)


def test_poisson_gradient_and_loss_per_element(case):
    irf = _irf(case["w"], case["c"], case["b"])
    for eps in FLOORS:
        loss4_ref, g64, bound, _ = LO.poisson_irf64(case["h"], case["target"], GT, case["w"], case["c"], case["b"], eps,
                                                    GS, y=case["lam"], A=case["A"])
        loss4, grad = _poisson(case["h"], case["target"], irf, eps)
        g = grad.cpu().numpy()
        gerr = np.abs(g.astype(np.float64) - g64)
        rel = np.abs(loss4.double().cpu().numpy() - loss4_ref) / np.maximum(np.abs(loss4_ref), 1e-300)
        print(f"rows {case['rows']} (nr, L, c) ({case['nr']}, {case['L']}, {case['c']}) b {float(case['b']):g} eps {eps:g}: "
              f"gradient err/bound {_share(gerr, bound):.3f}  loss4 rel {rel.max():.2e}")
        assert loss4_ref[2] > 0          # ([3], the counts, can be 0 where the response's mass lies past a short row:
        #                                  loss4[1] and [3] must then be exactly 0)
        assert np.isfinite(g).all() and np.all(gerr <= bound)
        assert _close4(loss4, loss4_ref)
        # want_grad=False: the same loss, no gradient written
        loss4_b, none = _poisson(case["h"], case["target"], irf, eps, want_grad=False)
        assert none is None and torch.equal(loss4_b, loss4)


def _irf_test_inputs(rows, nr, L, c, kind):
    """tests/test_gpu_irf.py's case inputs, restated."""
    g = np.random.default_rng(1000 * rows + nr + L)
    w = _gauss(L) if kind == "gauss" else g.standard_normal(L).astype(np.float32)
    h = (g.random((rows, nr)) * (g.random((rows, nr)) > 0.7)).astype(np.float32)
    target = (g.random((rows, nr)) * 1e-2).astype(np.float32)
    return w, h, target


@pytest.mark.parametrize("kind", ["gauss", "signed"])
@pytest.mark.parametrize("nr,L,c", IRF_SHAPES)
def test_mse_kind_is_nlosgr_mse_irf(nr, L, c, kind):
    """NLOSGR_LOSS_MSE through the new entry point == nlosgr_mse_irf bit for bit, whatever rate_floor holds."""
    from nlosgr import _lib
    from nlosgr.train import mse
    lib = _lib.load()
    for rows in ROWS:
        w, h, target = _irf_test_inputs(rows, nr, L, c, kind)
        irf = _irf(w, c, 0.01)
        x, t = torch.from_numpy(h).cuda(), torch.from_numpy(target).cuda()
        ref4, refg = mse(x, t, 100.0, grad_scale=0.5, raw=True, irf=irf)
        for floor, want_grad in [(float("nan"), True), (0.0, True), (1.0, False)]:
            out = torch.full((4,), 7.0, device="cuda:0")
            grad = torch.full_like(x, 7.0) if want_grad else None
            ws = torch.empty(lib.nlosgr_loss_irf_workspace_bytes(rows) // 4, dtype=torch.float32, device="cuda:0")
            s = irf.struct()
            spec = _lib.Loss(_lib.LOSS_MSE, floor)
            _lib.check(lib.nlosgr_loss_irf(_lib.ptr(x), _lib.ptr(t), 100.0, rows, nr, ctypes.byref(s), ctypes.byref(spec),
                                           0.5, _lib.ptr(grad), _lib.ptr(ws), _lib.ptr(out), _lib.stream_handle(x.device)))
            assert torch.equal(out, ref4)
            assert grad is None or torch.equal(grad, refg)
    # and nlosgr.loss.loss(kind="mse") is train.mse, with and without an IRF
    from nlosgr.loss import loss
    a4, ga = loss(x, t, 100.0, grad_scale=0.5, raw=True, irf=irf, kind="mse", rate_floor=float("nan"))
    assert torch.equal(a4, ref4) and torch.equal(ga, refg)
    a4, ga = loss(x, t, 100.0, grad_scale=0.5, raw=True)
    b4, gb = mse(x, t, 100.0, grad_scale=0.5, raw=True)
    assert torch.equal(a4, b4) and torch.equal(ga, gb)


@pytest.mark.parametrize("rows,nr,L,c", [(3, 63, 2, 1), (3, 1000, 255, 254), (5, 2049, 129, 64)])
def test_clamp_idle_with_signed_taps(rows, nr, L, c):
    """Signed taps on a background that keeps lambda more than 10 E above 0: the clamp never acts on either side, and
    the gradient stays within the bound."""
    g = np.random.default_rng(nr + L)
    w = g.standard_normal(L).astype(np.float32)
    h = (20.0 * g.random((rows, nr)) * (g.random((rows, nr)) > 0.7)).astype(np.float32)
    reach = IO.apply64(np.abs(h), np.abs(w), c, 0.0).max()
    b = np.float32(2.0 * reach + 1.0)
    lam = IO.apply64(h, w, c, b)
    E, A = IO.apply_bound(h, w, c, b)
    assert np.all(lam > 10.0 * E)
    target = _counts(g, lam)
    irf = _irf(w, c, b)
    for eps in FLOORS:
        loss4_ref, g64, bound, _ = LO.poisson_irf64(h, target, GT, w, c, b, eps, GS, y=lam, A=A)
        loss4, grad = _poisson(h, target, irf, eps)
        gerr = np.abs(grad.cpu().numpy().astype(np.float64) - g64)
        print(f"signed taps, rows {rows} (nr, L, c) ({nr}, {L}, {c}) eps {eps:g}: gradient err/bound {_share(gerr, bound):.3f}")
        assert np.all(gerr <= bound) and _close4(loss4, loss4_ref)


@pytest.mark.parametrize("rows,nr,L,c", [(4, 63, 2, 1), (6, 1000, 33, 16), (4, 2049, 129, 64)])
def test_clamp_acts_on_negative_rates(rows, nr, L, c):
    """Negative taps and b = 0: the even rows (h > 0) have lambda < -10 E throughout, the odd rows (h < 0) a positive
    lambda.  The clamped rows' gradient is exactly 0 and their deviance is 2 [y' log(y'/eps) - y' + eps]; the other
    rows stay within the bound."""
    g = np.random.default_rng(nr + L + 1)
    w = -_gauss(L)
    h = (1.0 + 20.0 * g.random((rows, nr))).astype(np.float32)
    h[1::2] *= -1.0
    lam = IO.apply64(h, w, c, 0.0)
    E, A = IO.apply_bound(h, w, c, 0.0)
    assert np.all(lam[0::2] < -10.0 * E[0::2]) and np.all(lam[1::2] > 10.0 * E[1::2])
    counts = g.poisson(np.abs(lam))
    irf = _irf(w, c, 0.0)
    for eps in FLOORS:
        # counts in units of 8 floors at the small floor, so y'/rho stays below 2^9 on the clamped rows: the fp32
        # e = r / y' lies within 2^-24 of -1 + rho/y', which log1pf sees as a relative 2^-24 y'/rho of its argument;
        # against log(y'/rho) - 1 that is 6e-8 * 512 / 5.2 = 6e-6 of an element's deviance at the worst, inside 1e-5
        target = (counts * min(1.0, 8.0 * eps) / GT).astype(np.float32)
        assert (GT * target.max() + eps) / eps < 512.0
        loss4_ref, g64, bound, _ = LO.poisson_irf64(h, target, GT, w, c, 0.0, eps, GS, y=lam, A=A)
        loss4, grad = _poisson(h, target, irf, eps)
        g32 = grad.cpu().numpy()
        assert not g32[0::2].any() and not g64[0::2].any()
        assert np.all(np.abs(g32.astype(np.float64) - g64) <= bound) and g32[1::2].any()
        assert _close4(loss4, loss4_ref)
        # the clamped rows alone: rho = eps
        e32 = float(np.float32(eps))
        yp = GT * target[0::2].astype(np.float64) + e32
        closed = float((2.0 * (yp * np.log(yp / e32) - yp + e32)).sum())
        only4, only_g = _poisson(np.ascontiguousarray(h[0::2]), np.ascontiguousarray(target[0::2]), irf, eps)
        assert abs(only4[2].item() - closed) <= 1e-5 * closed and not only_g.any()


def test_finite_inputs_give_no_nan():
    from nlosgr.loss import loss
    rows, nr, L, c = 5, 300, 33, 7
    g = np.random.default_rng(9)
    w = g.standard_normal(L).astype(np.float32)
    h = torch.from_numpy((20.0 * g.standard_normal((rows, nr))).astype(np.float32)).cuda()     # rates of either sign
    t = torch.from_numpy((30.0 * g.standard_normal((rows, nr))).astype(np.float32)).cuda()     # negative targets too
    t[0, :8] = 0.0
    h[1] = 0.0
    t[2] = 3.0e6                                                   # counts far above the rate
    for irf in (_irf(w, c, -0.5), _irf(_gauss(L), c, 0.0), None):
        for eps in FLOORS + [1e-30]:
            for gt in (1.0, -1.0):
                loss4, grad = loss(h, t, gt, raw=True, irf=irf, kind="poisson", rate_floor=eps)
                assert torch.isfinite(loss4).all() and torch.isfinite(grad).all()
                assert loss4[2] >= 0 and loss4[3] >= 0


def test_repeatable_and_row_split_bitwise():
    from nlosgr.loss import loss
    rows, nr, L, c = 257, 1000, 255, 254
    g = np.random.default_rng(5)
    w = _gauss(L)
    h = (20.0 * g.random((rows, nr)) * (g.random((rows, nr)) > 0.7)).astype(np.float32)
    target = torch.from_numpy(g.poisson(IO.apply64(h, w, c, 0.01)).astype(np.float32)).cuda()
    hist = torch.from_numpy(h).cuda()
    irf = _irf(w, c, 0.01)
    for eps in FLOORS:
        kw = dict(raw=True, irf=irf, kind="poisson", rate_floor=eps)
        # grad_scale = the call's own row count: every call then scales by 2 / nr exactly
        a4, ga = loss(hist, target, 1.0, grad_scale=float(rows), **kw)
        b4, gb = loss(hist, target, 1.0, grad_scale=float(rows), **kw)
        assert torch.equal(a4, b4) and torch.equal(ga, gb)
        lo4, glo = loss(hist[:128], target[:128], 1.0, grad_scale=128.0, **kw)
        hi4, ghi = loss(hist[128:], target[128:], 1.0, grad_scale=129.0, **kw)
        assert torch.equal(torch.cat([glo, ghi]), ga)
        assert torch.all((lo4[2:] + hi4[2:] - a4[2:]).abs() <= 1e-6 * a4[2:].abs())


def test_empty_and_no_irf():
    from nlosgr import _lib
    from nlosgr.loss import identity_irf, loss
    lib = _lib.load()
    dev = torch.device("cuda:0")
    e = torch.empty(0, 16, device=dev)
    loss2, grad = loss(e, e, kind="poisson")
    assert loss2.tolist() == [0.0, 0.0] and grad.numel() == 0
    out = torch.full((4,), 7.0, device=dev)
    ws = torch.empty(64, device=dev)
    taps = torch.ones(1, device=dev)
    i = ctypes.byref(_lib.Irf(1, 0, _lib.ptr(taps), 0.0))
    for kind in (_lib.LOSS_MSE, _lib.LOSS_POISSON):
        out.fill_(7.0)
        s = ctypes.byref(_lib.Loss(kind, 1.0))
        assert lib.nlosgr_loss_irf(None, None, 1.0, 0, 16, i, s, 1.0, None, _lib.ptr(ws), _lib.ptr(out), None) == 0
        torch.cuda.synchronize()
        assert out.tolist() == [0.0, 0.0, 0.0, 0.0]
    # no IRF: the cached identity IRF, bitwise the explicit one; any leading shape
    g = torch.Generator().manual_seed(4)
    hist = (torch.rand(7, 5, 300, generator=g) * 9).cuda()
    target = torch.poisson(torch.rand(7, 5, 300, generator=g) * 9, generator=g).cuda()
    for eps in FLOORS:
        a4, ga = loss(hist, target, 1.0, raw=True, kind="poisson", rate_floor=eps)
        b4, gb = loss(hist, target, 1.0, raw=True, kind="poisson", rate_floor=eps, irf=_irf([1.0], 0, 0.0))
        assert torch.equal(a4, b4) and torch.equal(ga, gb) and ga.shape == hist.shape
    assert identity_irf(dev) is identity_irf(dev)
    with pytest.raises(RuntimeError):                             # the IRF path's cap on the time axis
        loss(torch.zeros(1, 8193, device=dev), torch.zeros(1, 8193, device=dev), kind="poisson")


def test_simulate_capture_gpu():
    from nlosgr.irf import gaussian_irf
    from nlosgr.loss import simulate_capture
    g = torch.Generator().manual_seed(2)
    hist = (torch.rand(6, 200, generator=g) * (torch.rand(6, 200, generator=g) > 0.6) * 30).cuda()
    irf = gaussian_irf(5.0, tail_bins=2.0, background=0.2)
    N = 100000.0
    a, sa = simulate_capture(hist, irf, photons=N, generator=torch.Generator(device="cuda:0").manual_seed(1))
    b, sb = simulate_capture(hist, irf, photons=N, generator=torch.Generator(device="cuda:0").manual_seed(1))
    assert torch.equal(a, b) and sa == sb and a.is_cuda and a.dtype == torch.float32
    assert torch.all(a >= 0) and torch.equal(a, a.round())
    assert abs(a.double().sum().item() - N) <= 6.0 * N ** 0.5


def _scene_model(dev, mode, ng=400, H=6, W=5, T=48, seed=3, cutoff=3.0):
    """tests/test_gpu_train.py's _scene_model, restated (400 Gaussians, 6 x 5 wall, 48 bins)."""
    from nlosgr import GaussianParams
    from nlosgr.volume import Scene, make_config
    scene = Scene(H=H, W=W, T=T, ns=8)
    model = GaussianParams.synthetic(ng, 3, preset="cuda", device=dev, seed=seed)
    geo = scene.geometry(dev, "cuda", mode)
    cfg = make_config(model, scene, "cuda", mode, cutoff=cutoff)
    g = torch.Generator().manual_seed(seed + 1)
    target = (torch.rand(H * W, T, generator=g) * 1e-3).to(dev)
    return scene, model, geo, cfg, target


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("mode", ["noocl", "occl"])
def test_train_step_poisson_matches_torch_composition(monkeypatch, mode):
    """Three fused TrainStep(loss="poisson", irf=...) iterations == render autograd -> conv1d -> PoissonDeviance ->
    torch.optim.Adam (the tolerances of test_train_step_with_irf_matches_torch_composition).  occl: ray_cache=True
    takes _occl_step, forced to two wall-point batches."""
    from nlosgr import GaussianParams, train as T_
    from nlosgr.irf import gaussian_irf
    from nlosgr.loss import PoissonDeviance
    from nlosgr.render import tile_rows_bytes
    from nlosgr.volume import render_volume
    dev = torch.device("cuda:0")
    scene, model, geo, cfg, target = _scene_model(dev, mode)
    irf = gaussian_irf(6.0, tail_bins=3.0, background=2e-3)
    twin = GaussianParams(*(p.detach().clone() for p in model.parameters()), model.active_sh_degree)
    gt_times, floor = 100.0, 0.05
    crit = PoissonDeviance(floor)
    opt = T_.OptimizationParams()
    if mode == "occl":
        cfg = replace(cfg, ray_cache=True)
        monkeypatch.setattr(T_, "OCCL_BATCH_BYTES", 15 * tile_rows_bytes(geo) // geo.nwall)
    step = T_.TrainStep(model, geo, cfg, target, gt_times=gt_times, opt=opt, spatial_lr_scale=2.0, irf=irf,
                        keep_grads=True, loss="poisson", rate_floor=floor)
    if mode == "occl":
        assert len(step.occl_batches()) == 2
    names = ["mu", "scaling", "rotation", "opacity", "f_dc", "f_rest"]     # GaussianParams.parameters() order
    by_name = dict(zip(names, twin.parameters()))
    lr0 = {"mu": opt.position_lr_init * 2.0, "f_dc": opt.feature_lr, "f_rest": opt.feature_lr / 20.0,
           "opacity": opt.opacity_lr, "scaling": opt.scaling_lr, "rotation": opt.rotation_lr}
    order = ["mu", "f_dc", "f_rest", "opacity", "scaling", "rotation"]       # gaussian_model.py:229-236
    torch_opt = torch.optim.Adam([{"params": [by_name[n]], "lr": lr0[n], "name": n} for n in order], lr=0.0,
                                 eps=1e-15, foreach=False)
    L, c = len(irf), irf.center
    kern = irf.taps.to(dev).flip(0).view(1, 1, L)                 # conv1d correlates: flipped taps, pad (L-1-c, c)

    def through_irf(h):
        y = torch.nn.functional.conv1d(torch.nn.functional.pad(h.unsqueeze(1), (L - 1 - c, c)), kern).squeeze(1)
        return y + irf.background
    for it in range(3):
        loss2 = step(it)
        torch_opt.param_groups[0]["lr"] = step.learning_rates(it)[0]
        torch_opt.zero_grad()
        hist = render_volume(twin, geo, replace(cfg, ray_cache=False) if mode == "occl" else cfg)
        loss = crit(through_irf(hist), target * gt_times)
        loss.backward()
        torch_opt.step()
        if mode == "noocl" and it == 0:
            # keep_grads: self.hist is the render before the IRF, self.grad_hist is dL/dhist of ITS loss
            assert _rel(step.hist, hist) <= 1e-5
            hd = step.hist.detach().clone().requires_grad_(True)
            (gh,) = torch.autograd.grad(crit(through_irf(hd), target * gt_times), hd)
            assert _rel(step.grad_hist, gh) <= 1e-5
        print(f"{mode} iteration {it}: loss {loss2[0].item():.6e}  rel to torch {abs(loss2[0].item() - loss.item()) / loss.item():.2e}")
        assert abs(loss2[0].item() - loss.item()) <= 1e-5 * loss.item()
        count = (target * gt_times).clamp_min(0).double().sum().item()
        assert abs(loss2[1].item() - loss.item() * target.numel() / count) <= 1e-5 * loss2[1].item()
    torch.cuda.synchronize()
    for n, a, b in zip(names, model.parameters(), twin.parameters()):
        print(f"{mode} {n}: rel {_rel(a, b):.2e}")
        assert _rel(a, b) <= 1e-5, n
