"""GPU checks of the temporal instrument response (include/nlosgr.h ABI 12, csrc/nlosgr_irf.hip) against the
float64 oracle of tests/irf_oracle.py, per element and under derived bounds:

  apply / adjoint   |y - y64| <= (L + 2) 2^-24 A,  A = |b| + (|w| * |h|): the running-error bound of an L-term
                    fp32 sum in any order; bins with A = 0 must come out exactly b
  fused gradient    |g - g64| <= (2L + 8) 2^-24 S,  S = gscale adjoint_|w|(A + |gt target|)
  fused loss        loss, equal_loss to 1e-5 relative (the project's number for nlosgr_mse)
  identity IRF      grad_out bitwise nlosgr_mse's, loss to 1e-6
  repeatability     two runs bitwise; rows [0,128) + [128,257) bitwise the whole call's gradient rows
  errors            bad arguments -> a code and a message, nothing launched
  convolve_time     backward == the adjoint call; forward within the apply bound of the CPU fallback
  TrainStep(irf=)   == render -> conv1d -> MSE -> torch.optim.Adam over 3 iterations (whole wall, and the
                    occlusion mode's wall-point batches)

Shapes: a row shorter than the IRF, nr on either side of a wave and of the workgroup's span, the centre at
either end, a ragged last row block, the tap limit and the row-length limit.  `-s` prints the worst measured
share of each bound per case.
"""
import ctypes
from dataclasses import replace

import numpy as np
import pytest
import torch

import irf_oracle as IO

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 257]
SHAPES = [(1, 1, 0), (7, 33, 16), (63, 2, 1), (65, 255, 0), (1000, 255, 254), (1024, 512, 100), (8192, 129, 64)]
KINDS = ["gauss", "signed"]
B = 0.01
CASES = [(r, nr, L, c, k) for k in KINDS for (nr, L, c) in SHAPES for r in ROWS]


def _taps(L, kind, g):
    if kind == "gauss":       # a normalised Gaussian over the L taps (its peak is not at c: c comes from the case)
        k = np.arange(L, dtype=np.float64)
        w = np.exp(-0.5 * ((k - (L - 1) / 2) / (L / 8 + 0.5)) ** 2)
        return (w / w.sum()).astype(np.float32)
    return g.standard_normal(L).astype(np.float32)


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"r{p[0]}-nr{p[1]}-L{p[2]}-c{p[3]}-{p[4]}")
def case(request):
    """Inputs (70 % exact zeros in h) and the float64 apply of one case, shared by the tests that use it."""
    rows, nr, L, c, kind = request.param
    g = np.random.default_rng(1000 * rows + nr + L)
    w = _taps(L, kind, g)
    h = (g.random((rows, nr)) * (g.random((rows, nr)) > 0.7)).astype(np.float32)
    target = (g.random((rows, nr)) * 1e-2).astype(np.float32)
    y64 = IO.apply64(h, w, c, np.float32(B))
    bound, A = IO.apply_bound(h, w, c, np.float32(B))
    return dict(rows=rows, nr=nr, L=L, c=c, kind=kind, w=w, h=h, target=target, y64=y64, bound=bound, A=A)


def _irf(w, c, b=0.0):
    from nlosgr.irf import IRF
    return IRF(torch.from_numpy(np.asarray(w, dtype=np.float32)), c, b).to("cuda:0")


def _name(case):
    return f"rows {case['rows']} (nr, L, c) ({case['nr']}, {case['L']}, {case['c']}) {case['kind']}"


def _share(err, bound):
    m = bound > 0
    return float((err[m] / bound[m]).max()) if m.any() else 0.0


def test_apply_and_adjoint_per_element(case):
    from nlosgr.irf import irf_apply
    irf = _irf(case["w"], case["c"], B)
    x = torch.from_numpy(case["h"]).cuda()
    y = irf_apply(x, irf, False).cpu().numpy()
    err = np.abs(y.astype(np.float64) - case["y64"])
    a_share = _share(err, case["bound"])
    dark = case["A"] == abs(np.float64(np.float32(B)))          # no light reaches the bin: exactly b
    assert np.array_equal(y[dark], np.full(int(dark.sum()), np.float32(B)))
    g = irf_apply(x, irf, True).cpu().numpy()
    g64 = IO.adjoint64(case["h"], case["w"], case["c"])
    gbound, GA = IO.adjoint_bound(case["h"], case["w"], case["c"])
    gerr = np.abs(g.astype(np.float64) - g64)
    print(f"{_name(case)}: apply err/bound {a_share:.3f}  adjoint err/bound {_share(gerr, gbound):.3f}")
    assert np.all(err <= case["bound"])
    assert np.all(gerr <= gbound)
    assert not g[GA == 0].any()                                  # the adjoint adds no background


def test_fused_gradient_per_element(case):
    from nlosgr.train import mse
    irf = _irf(case["w"], case["c"], B)
    gt, gs = 100.0, 0.5
    loss4_ref, g64, gbound = IO.mse_irf64(case["h"], case["target"], gt, case["w"], case["c"], np.float32(B), gs,
                                           y=case["y64"], A=case["A"])
    loss4, grad = mse(torch.from_numpy(case["h"]).cuda(), torch.from_numpy(case["target"]).cuda(), gt, grad_scale=gs,
                      raw=True, irf=irf)
    gerr = np.abs(grad.cpu().numpy().astype(np.float64) - g64)
    print(f"{_name(case)}: fused gradient err/bound {_share(gerr, gbound):.3f}")
    assert np.all(gerr <= gbound)
    assert np.all(np.abs(loss4.cpu().numpy() - loss4_ref) <= 1e-5 * np.abs(loss4_ref))
    # want_grad=False: the same loss, no gradient written
    loss4_b, none = mse(torch.from_numpy(case["h"]).cuda(), torch.from_numpy(case["target"]).cuda(), gt, grad_scale=gs,
                        want_grad=False, raw=True, irf=irf)
    assert none is None and torch.equal(loss4_b, loss4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nr,L,c", SHAPES)
@pytest.mark.parametrize("rows", [1, 257])
def test_fused_loss_values(rows, nr, L, c, kind):
    """The inputs of test_mse_matches_torch (hist ~ U(0,1), target ~ 1e-2 U, gt_times 100): d does not cancel."""
    from nlosgr.train import mse
    g = torch.Generator(device="cpu").manual_seed(rows * nr + L)
    hist = torch.rand(rows, nr, generator=g)
    target = torch.rand(rows, nr, generator=g) * 1e-2
    w = _taps(L, kind, np.random.default_rng(L))
    ref = IO.loss_irf64(hist.numpy(), target.numpy(), 100.0, w, c, np.float32(B))
    loss2, _ = mse(hist.cuda(), target.cuda(), 100.0, irf=_irf(w, c, B), want_grad=False)
    rel = np.abs(loss2.cpu().numpy() - ref) / ref
    print(f"rows {rows} (nr, L, c) ({nr}, {L}, {c}) {kind}: loss rel {rel[0]:.2e}  equal_loss rel {rel[1]:.2e}")
    assert rel[0] <= 1e-5 and rel[1] <= 1e-5


@pytest.mark.parametrize("rows,nr", [(1, 1), (3, 1000), (257, 1031), (5, 8192), (300, 48)])
def test_identity_irf_is_nlosgr_mse(rows, nr):
    from nlosgr.train import mse
    g = torch.Generator(device="cpu").manual_seed(rows + nr)
    hist = torch.rand(rows, nr, generator=g).cuda()
    target = (torch.rand(rows, nr, generator=g) * 1e-2).cuda()
    a4, ga = mse(hist, target, 100.0, grad_scale=0.5, raw=True)
    b4, gb = mse(hist, target, 100.0, grad_scale=0.5, raw=True, irf=_irf([1.0], 0, 0.0))
    assert torch.equal(ga, gb)                                    # fma(1, h, 0) = h
    assert torch.all((a4 - b4).abs() <= 1e-6 * a4.abs())


def test_repeatable_and_row_split_bitwise():
    from nlosgr.train import mse
    rows, nr, L, c = 257, 1000, 255, 254
    g = np.random.default_rng(5)
    hist = torch.from_numpy(g.random((rows, nr)).astype(np.float32)).cuda()
    target = torch.from_numpy((g.random((rows, nr)) * 1e-2).astype(np.float32)).cuda()
    irf = _irf(g.standard_normal(L), c, B)
    # grad_scale = the call's own row count: every call then scales d by 2 / nr exactly
    a4, ga = mse(hist, target, 100.0, grad_scale=float(rows), raw=True, irf=irf)
    b4, gb = mse(hist, target, 100.0, grad_scale=float(rows), raw=True, irf=irf)
    assert torch.equal(a4, b4) and torch.equal(ga, gb)
    lo4, glo = mse(hist[:128], target[:128], 100.0, grad_scale=128.0, raw=True, irf=irf)
    hi4, ghi = mse(hist[128:], target[128:], 100.0, grad_scale=129.0, raw=True, irf=irf)
    assert torch.equal(torch.cat([glo, ghi]), ga)
    assert torch.all((lo4[2:] + hi4[2:] - a4[2:]).abs() <= 1e-6 * a4[2:].abs())


def test_errors_and_empty():
    from nlosgr import _lib
    from nlosgr.train import mse
    lib = _lib.load()
    dev = torch.device("cuda:0")
    taps = torch.ones(8, device=dev)
    x = torch.zeros(2, 16, device=dev)
    y = torch.empty_like(x)
    ws = torch.empty(64, device=dev)
    out = torch.empty(4, device=dev)
    P = _lib.ptr

    def irf(ntaps=8, center=0, t=taps):
        return ctypes.byref(_lib.Irf(ntaps, center, P(t), 0.0))

    def both(i, rows=2, nr=16):
        return (lib.nlosgr_irf_apply(P(x), rows, nr, i, 0, P(y), None),
                lib.nlosgr_mse_irf(P(x), P(x), 1.0, rows, nr, i, 1.0, P(y), P(ws), P(out), None))
    for i, word in [(irf(ntaps=0), b"ntaps"), (irf(ntaps=513), b"ntaps"), (irf(center=8), b"center"),
                    (irf(center=-1), b"center"), (irf(t=None), b"taps")]:
        for rc in both(i):
            assert rc == 1 and word in lib.nlosgr_last_error()
    for rc in both(irf(), rows=-1):
        assert rc == 1 and b"rows" in lib.nlosgr_last_error()
    for rc in both(irf(), nr=0):
        assert rc == 1 and b"nr" in lib.nlosgr_last_error()
    for rc in both(irf(), nr=_lib.IRF_MAX_NR + 1):
        assert rc == 3 and b"nr" in lib.nlosgr_last_error()     # NLOSGR_E_UNSUPPORTED, never a wrong result
    assert lib.nlosgr_irf_apply(None, 2, 16, irf(), 0, P(y), None) == 1
    assert lib.nlosgr_mse_irf(P(x), P(x), 1.0, 2, 16, irf(), 1.0, P(y), None, P(out), None) == 1
    assert lib.nlosgr_mse_irf(P(x), P(x), 1.0, 2, 16, None, 1.0, P(y), P(ws), P(out), None) == 1
    # rows == 0: zeros, as nlosgr_mse gives for n == 0
    out.fill_(7.0)
    assert lib.nlosgr_mse_irf(None, None, 1.0, 0, 16, irf(), 1.0, None, P(ws), P(out), None) == 0
    assert lib.nlosgr_irf_apply(None, 0, 16, irf(), 0, None, None) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0.0, 0.0, 0.0, 0.0]
    e = torch.empty(0, 16, device=dev)
    loss2, grad = mse(e, e, irf=_irf(np.ones(8), 0))
    assert loss2.tolist() == [0.0, 0.0] and grad.numel() == 0
    assert lib.nlosgr_mse_irf_workspace_bytes(0) > 0 and lib.nlosgr_mse_irf_workspace_bytes(1000) >= 8000


def test_convolve_time_gpu():
    from nlosgr.irf import adjoint_time, convolve_time, gaussian_irf, irf_apply
    rows, nr = 5, 300
    g = torch.Generator().manual_seed(2)
    irf = gaussian_irf(9.0, tail_bins=4.0, background=0.02)
    h = torch.rand(rows, nr, generator=g) * (torch.rand(rows, nr, generator=g) > 0.7)
    z = torch.randn(rows, nr, generator=g)
    x = h.cuda().requires_grad_(True)
    y = convolve_time(x, irf)
    (gx,) = torch.autograd.grad(y, x, z.cuda())
    assert torch.equal(gx, irf_apply(z.cuda(), irf, True)) and torch.equal(gx, adjoint_time(z.cuda(), irf))
    w = irf.taps.numpy()
    y_cpu = convolve_time(h.double(), irf).numpy()                # the CPU fallback, in float64
    bound, _ = IO.apply_bound(h.numpy(), w, irf.center, np.float32(irf.background))
    assert np.all(np.abs(y.detach().cpu().numpy().astype(np.float64) - y_cpu) <= bound)
    g_cpu = adjoint_time(z.double(), irf).numpy()
    gbound, _ = IO.adjoint_bound(z.numpy(), w, irf.center)
    assert np.all(np.abs(gx.cpu().numpy().astype(np.float64) - g_cpu) <= gbound)
    # any leading shape, one row
    assert torch.equal(convolve_time(x.detach()[0], irf), y.detach()[0])
    assert torch.equal(convolve_time(x.detach().view(5, 1, nr), irf).view(5, nr), y.detach())


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
def test_train_step_with_irf_matches_torch_composition(monkeypatch, mode):
    """Three fused TrainStep(irf=...) iterations == render autograd -> conv1d -> torch MSE -> torch.optim.Adam
    (the existing composition test's tolerances).  occl: ray_cache=True takes _occl_step, forced to two
    wall-point batches."""
    from nlosgr import GaussianParams, train as T_
    from nlosgr.irf import gaussian_irf
    from nlosgr.render import tile_rows_bytes
    from nlosgr.volume import render_volume
    dev = torch.device("cuda:0")
    scene, model, geo, cfg, target = _scene_model(dev, mode)
    irf = gaussian_irf(6.0, tail_bins=3.0, background=2e-3)
    twin = GaussianParams(*(p.detach().clone() for p in model.parameters()), model.active_sh_degree)
    gt_times = 100.0
    opt = T_.OptimizationParams()
    if mode == "occl":
        cfg = replace(cfg, ray_cache=True)
        monkeypatch.setattr(T_, "OCCL_BATCH_BYTES", 15 * tile_rows_bytes(geo) // geo.nwall)
    step = T_.TrainStep(model, geo, cfg, target, gt_times=gt_times, opt=opt, spatial_lr_scale=2.0, irf=irf,
                        keep_grads=True)
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
    for it in range(3):
        loss2 = step(it)
        torch_opt.param_groups[0]["lr"] = step.learning_rates(it)[0]
        torch_opt.zero_grad()
        hist = render_volume(twin, geo, replace(cfg, ray_cache=False) if mode == "occl" else cfg)
        y = torch.nn.functional.conv1d(torch.nn.functional.pad(hist.unsqueeze(1), (L - 1 - c, c)), kern).squeeze(1)
        y = y + irf.background
        loss = ((y - target * gt_times) ** 2).mean()
        loss.backward()
        torch_opt.step()
        if mode == "noocl" and it == 0:
            # keep_grads: self.hist is the render before the IRF, self.grad_hist is dL/dhist of ITS loss
            # (fp32 sums in another order, as everywhere in this comparison: 1e-5 of the maximum)
            assert _rel(step.hist, hist) <= 1e-5
            hd = step.hist.detach().clone().requires_grad_(True)
            yd = torch.nn.functional.conv1d(torch.nn.functional.pad(hd.unsqueeze(1), (L - 1 - c, c)), kern).squeeze(1)
            (gh,) = torch.autograd.grad(((yd + irf.background - target * gt_times) ** 2).mean(), hd)
            assert _rel(step.grad_hist, gh) <= 1e-5
        assert abs(loss2[0].item() - loss.item()) <= 1e-5 * loss.item()
    torch.cuda.synchronize()
    for n, a, b in zip(names, model.parameters(), twin.parameters()):
        assert _rel(a, b) <= 1e-5, n
