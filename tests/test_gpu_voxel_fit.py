"""GPU tests of the voxel-domain fit (nlosgr.voxel_fit.VoxelFitStep) at small shapes: 16 Gaussians, a 16^3 grid,
6 x 6 sensed points on the wall, nr = 64.

Volume mode: five steps against the same fit in float64 (voxel_grad_oracle.volumes64 + torch.optim.Adam with the
step's betas, eps and learning rates).  Capture mode (confocal, one laser spot, a spot per measurement; power 2):
one step's gradients against the float64 composition  volumes64 -> forward64 -> dMSE/drows -> backproject64 -> G_a ->
voxel_grad_oracle.reference,  per Gaussian, e_g <= tol s_g as in test_gpu_voxelize_bwd.py.

Tolerances: 4 x the deviations measured on gfx950 (MI355X), rounded up to one significant digit.  Measured:

    volume mode   objective, relative deviation of steps 1..5: 1.4e-7 1.3e-6 1.7e-6 7.0e-7 5.6e-7  -> 7e-6
                  parameters after step 5, max |gpu - float64| / (5 lr): mu 8.8e-5, f_dc 4.5e-6, f_rest 2.0e-5,
                  opacity 1.0e-6, scaling 1.4e-5, rotation 4.7e-5                                    -> 4e-4
    capture mode  worst e_g / s_g        mu      scaling  rotation  opacity  features
                  confocal               1.5e-6  1.0e-6   6.7e-6    1.1e-6   1.1e-6
                  one laser spot         1.8e-6  7.2e-7   4.3e-6    4.5e-7   5.5e-7
                  a spot per measurement 3.2e-6  6.7e-7   3.4e-6    7.9e-7   7.6e-7                  -> 3e-5
"""
import numpy as np
import pytest
import torch

import backproject_oracle as BO
import forward_project_oracle as FO
import nonconfocal_oracle as NO
import voxel_grad_oracle as GO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NG, RES, NR = 16, 16, 64
R0, DR, POWER = 0.2, 0.0125, 2
CAM = (0.0, 0.0, 0.0)
CUTOFF = 5.7       # a pair the fp32 mask and the float64 mask disagree on weighs exp(-5.7^2 / 2) = 9e-8: below fp32 resolution
VOLUME_OBJ_RTOL = 7e-6
VOLUME_PARAM_TOL = 4e-4      # of 5 lr, the distance a parameter can move in 5 steps
CAPTURE_TOL = 3e-5


def _params(seed, shift=False):
    """16 generic cuda-preset Gaussians inside the grid (SH degree 1): anisotropic, rotated, std 0.04 .. 0.08, so
    no gradient entry is zero by symmetry.  shift: the start of the fit, mu moved by half a voxel, opacity offset."""
    g = torch.Generator().manual_seed(seed)
    mu = (torch.rand(NG, 3, generator=g) - 0.5) * 0.3 + torch.tensor([0.0, 0.5, 0.0])
    scaling = torch.log(0.04 + 0.04 * torch.rand(NG, 3, generator=g))
    rotation = torch.randn(NG, 4, generator=g)
    opacity = torch.randn(NG, 1, generator=g) * 0.5
    fdc = ((0.2 + 0.6 * torch.rand(NG, 1, 1, generator=g)) - 0.5) / GO.R.C0
    frest = 0.1 * torch.randn(NG, 3, 1, generator=g)
    if shift:
        h = 0.5 / (RES - 1)
        mu = mu + 0.5 * h * torch.tensor([1.0, -1.0, 1.0])
        opacity = opacity + 0.3
    return dict(mu=mu, scaling=scaling, rotation=rotation, opacity=opacity, features_dc=fdc, features_rest=frest)


def _model(p, deg=1):
    from nlosgr import GaussianParams
    t = lambda k: torch.as_tensor(p[k]).float().to(DEV).contiguous()
    return GaussianParams(t("mu"), t("scaling"), t("rotation"), t("opacity"), t("features_dc"), t("features_rest"),
                          deg, deg)


def _grid():
    from nlosgr.voxelize import VoxelGrid
    return VoxelGrid((0.0, 0.5, 0.0), 0.5, RES)


def _walls():
    u = torch.linspace(-0.4, 0.4, 6)
    return torch.stack(torch.meshgrid(u, torch.zeros(1), u, indexing="ij"), -1).reshape(-1, 3).contiguous()


def _lasers(kind, walls):
    if kind == "confocal":
        return None
    if kind == "one":
        return torch.tensor([[0.15, 0.0, -0.25]])
    if kind == "same":
        return walls.clone()
    g = torch.Generator().manual_seed(8)
    return torch.cat(((torch.rand(36, 1, generator=g) - 0.5) * 0.8, torch.zeros(36, 1),
                      (torch.rand(36, 1, generator=g) - 0.5) * 0.8), dim=1)


def test_volume_mode_follows_the_float64_fit():
    from nlosgr.voxel_fit import VoxelFitStep
    from nlosgr.voxelize import voxelize
    grid = _grid()
    cam = torch.tensor(CAM, device=DEV)
    gt, start = _params(1), _params(1, shift=True)
    _, target = voxelize(_model(gt), grid, cam, preset="cuda", cutoff=CUTOFF, want_density=False)
    model = _model(start)
    step = VoxelFitStep(model, grid, cam, preset="cuda", cutoff=CUTOFF, target_volume=target)
    # the same fit in float64
    P = GO.params64(start, 1)
    leaves = [P._mu, P._features_dc, P._features_rest, P._opacity, P._scaling, P._rotation]      # train.GROUPS order
    opt = torch.optim.Adam([{"params": [t], "lr": 1.0} for t in leaves], betas=step.adam.betas, eps=step.adam.eps)
    t64 = target.cpu().double()
    coords = grid.coords()
    obj, ref = [], []
    for it in range(5):
        for grp, lr in zip(opt.param_groups, step.learning_rates(it)):
            grp["lr"] = lr
        opt.zero_grad()
        _, alb = GO.volumes64(P, coords, CAM, "cuda", 1.0, CUTOFF)
        L = (alb - t64).square().mean()
        L.backward()
        opt.step()
        ref.append(L.item())
        obj.append(step())
    obj = torch.stack(obj)[:, 0].cpu().double().numpy()
    ref = np.array(ref)
    rel = np.abs(obj - ref) / ref
    print("objectives", obj, "float64", ref, "relative deviation", rel)
    assert step.iteration == 5 and ref[-1] < ref[0]
    worst = {}
    lrs = step.learning_rates(0)
    got = [model._mu, model._features_dc, model._features_rest, model._opacity, model._scaling, model._rotation]
    from nlosgr.train import GROUPS
    for name, a, b, lr, p0 in zip(GROUPS, got, leaves, lrs, (start["mu"], start["features_dc"], start["features_rest"],
                                                              start["opacity"], start["scaling"], start["rotation"])):
        moved = (b.detach() - p0.double()).abs().max().item()
        worst[name] = (a.detach().cpu().double() - b.detach()).abs().max().item() / (5 * lr)
        print(f"{name:9s} deviation / (5 lr) = {worst[name]:.3e}   (moved {moved / (5 * lr):.3f} of 5 lr)")
        assert moved > 0.5 * lr
    assert rel.max() <= VOLUME_OBJ_RTOL
    assert max(worst.values()) <= VOLUME_PARAM_TOL, worst


@pytest.fixture(scope="module")
def capture():
    """The capture of the ground-truth Gaussians (power 2, projected on the GPU) per laser layout, and the start."""
    from nlosgr.forward_project import forward_project
    from nlosgr.voxelize import voxelize
    grid = _grid()
    cam = torch.tensor(CAM, device=DEV)
    walls = _walls().to(DEV)
    gt, start = _params(2), _params(2, shift=True)
    _, vol = voxelize(_model(gt), grid, cam, preset="cuda", cutoff=CUTOFF, want_density=False)
    out = {"grid": grid, "cam": cam, "walls": walls, "start": start, "scale": 0.37}
    for kind in ("confocal", "one", "each", "same"):
        ls = _lasers(kind, walls.cpu())
        ls = None if ls is None else ls.to(DEV)
        out[kind] = (ls, forward_project(vol, walls, grid, R0, DR, NR, power=POWER, lasers=ls).mul_(out["scale"]))
    return out


def _step(capture, kind, **kw):
    from nlosgr.voxel_fit import VoxelFitStep
    ls, rows = capture[kind]
    model = _model(capture["start"])
    step = VoxelFitStep(model, capture["grid"], capture["cam"], preset="cuda", cutoff=CUTOFF, rows=rows,
                        walls=capture["walls"], r0=R0, dr=DR, power=POWER, lasers=ls, volume_scale=capture["scale"],
                        keep_grads=True, **kw)
    return model, step


def _five(grads):
    d_mu, d_dc, d_rest, d_o, d_s, d_q = grads            # train.GROUPS order
    return (d_mu, d_s, d_q, d_o.reshape(-1), torch.cat((d_dc.reshape(NG, -1), d_rest.reshape(NG, -1)), dim=1))


@pytest.mark.parametrize("kind", ["confocal", "one", "each"])
def test_capture_mode_gradients_match_the_float64_chain(capture, kind):
    from nlosgr.backproject import fp32_window
    model, step = _step(capture, kind)
    loss2 = step()
    got = GO.as_named(_five(step.grads))
    # float64: volume -> rows -> dMSE/drows -> back-projection -> G_a -> the voxelizer's gradients
    grid, walls = capture["grid"], capture["walls"].cpu().numpy()
    ls, rows = capture[kind]
    tabs = [t.numpy() for t in grid.tables]
    r0, inv_dr = fp32_window(R0, DR)
    P = GO.params64(capture["start"], 1)
    with torch.no_grad():
        _, alb = GO.volumes64(P, grid.coords(), CAM, "cuda", 1.0, CUTOFF)
    s = capture["scale"]
    if ls is None:
        pred, _ = FO.forward64(alb.numpy(), walls, *tabs, r0, inv_dr, NR, POWER, want_bound=False)
    else:
        pred, _ = NO.forward64(alb.numpy(), walls, ls.cpu().numpy(), *tabs, r0, inv_dr, NR, POWER, want_bound=False)
    res = s * pred - rows.cpu().double().numpy()
    g_rows = 2.0 * res / res.size
    if ls is None:
        g_vol, _ = BO.backproject64(g_rows, walls, *tabs, r0, inv_dr, POWER, want_bound=False)
    else:
        g_vol, _ = NO.backproject64(g_rows, walls, ls.cpu().numpy(), *tabs, r0, inv_dr, POWER, want_bound=False)
    mse = float((res ** 2).mean())
    print(f"{kind}: MSE {loss2[0].item():.6e} float64 {mse:.6e}")
    grads, scale = GO.reference(P, grid.coords(), CAM, "cuda", None, torch.from_numpy(s * g_vol), mc=CUTOFF)
    r = GO.ratios(got, grads, scale, RES ** 3)
    for n in GO.NAMES:
        g = int(torch.argmax(r[n]))
        print(f"worst ratio {n:9s} {kind:8s}: {r[n][g].item():.3e} (Gaussian {g}, s_g {scale[n][g].item():.3e})")
    for n in GO.NAMES:
        assert grads[n].abs().max() > 0 and r[n].max() <= CAPTURE_TOL, (n, r[n].max().item())


def test_lasers_on_the_sensed_points_give_the_confocal_step(capture):
    """lasers == walls at power 2: the non-confocal operators reduce to the confocal ones, so the step's gradients
    are the confocal step's bitwise."""
    _, a = _step(capture, "confocal")
    _, b = _step(capture, "same")
    assert torch.equal(capture["confocal"][1], capture["same"][1])
    la, lb = a(), b()
    assert torch.equal(la, lb)
    for x, y in zip(a.grads, b.grads):
        assert torch.equal(x, y)


def test_density_control_rebinds_the_step(capture):
    """densify.add_new_gs(train_step=step) grows the model and rebinds the step; the next step runs on, and updates,
    the grown tensors."""
    from nlosgr import densify
    from nlosgr.voxel_fit import VoxelFitStep
    n0 = 40                              # add_new_gs grows by 5 %: 16 Gaussians would gain none
    a, b, c = capture["start"], _params(5), _params(6)
    model = _model({k: torch.cat((a[k], b[k], c[k][:8]), dim=0) for k in a})
    ls, rows = capture["one"]
    step = VoxelFitStep(model, capture["grid"], capture["cam"], preset="cuda", cutoff=CUTOFF, rows=rows,
                        walls=capture["walls"], r0=R0, dr=DR, power=POWER, lasers=ls, volume_scale=capture["scale"],
                        keep_grads=True)
    step()
    added = densify.add_new_gs(model, 64, train_step=step)
    assert added == 2 and model._mu.shape[0] == n0 + added
    assert step._tensors[0].data_ptr() == model._mu.data_ptr() and step.adam.exp_avg[0].shape == model._mu.shape
    before = [t.detach().clone() for t in model.parameters()]
    step()
    assert step.iteration == 2 and step.adam.step_count == 2 and step.grads[0].shape == model._mu.shape
    for b, t in zip(before, model.parameters()):
        assert t.shape[0] == n0 + added and not torch.equal(b, t.detach())
        assert (b[n0:] != t.detach()[n0:]).any()                        # the new rows are among the updated ones
    dead = torch.zeros(n0 + added, dtype=torch.bool, device=DEV)
    dead[3] = True
    densify.relocate_gs(model, dead, train_step=step)
    assert torch.isfinite(step()).all()


def test_poisson_loss_through_an_irf(capture):
    """loss="poisson" with an IRF runs, and the step's loss is loss.loss applied to the step's own projected rows."""
    from nlosgr.irf import IRF
    from nlosgr.loss import loss as fused_loss
    irf = IRF(torch.tensor([0.2, 0.5, 0.3]), 1, 0.05)
    model, step = _step(capture, "each", irf=irf, loss="poisson", rate_floor=0.5, gt_times=40.0)
    before = model._mu.detach().clone()
    loss2 = step()
    want, _ = fused_loss(step.rows_pred, capture["each"][1], 40.0, irf=irf.to(DEV), kind="poisson", rate_floor=0.5)
    assert torch.equal(loss2, want) and torch.isfinite(loss2).all() and loss2[0] > 0
    assert all(torch.isfinite(g).all() for g in step.grads) and not torch.equal(before, model._mu.detach())


def test_command_line_fits_a_non_confocal_capture(tmp_path, capture):
    """python -m nlosgr.voxel_fit (its main(), in process) on a capture file with one laser spot: the initial
    Gaussians come from the back-projection, the checkpoint goes through nlosgr.checkpoint and carries the step's
    Adam state, and --recon holds the nlosgr.voxelize keys on the fit's grid."""
    from nlosgr.checkpoint import load_checkpoint
    from nlosgr.data import make_data_kwargs, save_zaragoza
    from nlosgr.voxel_fit import main
    from nlosgr.voxelize import voxelize
    ls, rows = capture["one"]
    data = np.zeros((80, 6, 6), dtype=np.float32)
    data[16:80] = rows.cpu().numpy().T.reshape(NR, 6, 6)                 # bin 16 is r0 = 16 dr
    cap, ck, recon = str(tmp_path / "cap.mat"), str(tmp_path / "fit.pth"), str(tmp_path / "recon.npz")
    save_zaragoza(cap, data, capture["walls"].cpu().numpy().T, (0.0, 0.5, 0.0), 0.5, DR, 1.0,
                  laser_grid_positions=ls.cpu().numpy().T)
    dk, *_ = make_data_kwargs(cap, DEV, shuffle=False)
    assert tuple(dk["laser_grid_positions"].shape) == (3, 1)
    torch.manual_seed(0)
    np.random.seed(0)
    main([cap, "--resolution", str(RES), "--start", "16", "--end", "80", "--gaussians", "24", "--iterations", "4",
          "--power", str(POWER), "--cutoff", "3", "--out", ck, "--recon", recon])
    saved = torch.load(ck, map_location="cpu", weights_only=True)
    assert saved["iteration"] == 4 and saved["mu"].shape == (24, 3) and len(saved["optimizer"]["state"]) == 6
    model = load_checkpoint(ck, device=DEV)
    z = np.load(recon)
    assert sorted(z.files) == sorted(["density", "albedo", "front", "depth", "xs", "ys", "zs", "cam"])
    assert z["density"].shape == (RES, RES, RES) and np.isfinite(z["albedo"]).all() and z["albedo"].max() > 0
    dens, alb = voxelize(model, capture["grid"], torch.tensor(z["cam"], device=DEV), preset="cuda", cutoff=3.0)
    assert np.array_equal(z["density"], dens.cpu().numpy()) and np.array_equal(z["albedo"], alb.cpu().numpy())
    assert np.array_equal(z["front"], z["albedo"].max(axis=1))
