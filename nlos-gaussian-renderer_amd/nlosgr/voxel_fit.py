"""Fitting Gaussians to objectives on the voxel grid: the counterpart of train.TrainStep for the chain

    Gaussians -> voxelize (albedo_density) -> [forward_project -> fused loss -> backproject] -> nlosgr_voxelize_bwd

Two objectives:
  volume    the MSE of albedo_density against a given volume: distils a Landweber or back-projection volume into
            Gaussians instead of sampling from it.
  capture   the fused loss (MSE or Poisson deviance, through the capture's IRF) of volume_scale * A_power(
            albedo_density) against the capture's rows, A the forward projector (power 0..4, the range of its
            adjoint).  `lasers=` makes it a non-confocal capture: this is how such a capture is fitted with
            Gaussians, since the pair-major renderer is confocal only (data.volume_geometry raises for it).
            `operator=` (an nlosgr.lct.LctOperator) replaces the pair A, A^T by the LCT operator pair: a confocal
            capture on a wall lattice, fitted on the lattice's own voxels at FFT speed (fit_capture projector="lct").

VoxelFitStep runs one iteration per call with every piece on the device and no host synchronisation inside:
voxelize (albedo only) -> project -> loss and dL/drows -> back-project -> voxelize backward -> nlosgr_adam, with
TrainStep's learning-rate schedule, Adam, regulariser, rebind() and iteration counter, so densify.relocate_gs /
add_new_gs(train_step=) and checkpoint.save_checkpoint(train_step=) take it as they take a TrainStep.

    python -m nlosgr.voxel_fit CAPTURE.mat --resolution R --start S --end E --gaussians N --iterations I
        [--power P --falloff Q --cutoff C] [--projector lct [--nv N]] --out CKPT [--recon recon.npz]
"""
import argparse
import math

import numpy as np
import torch

from . import _lib
from .backproject import _gpu_f32, _lasers_arg, backproject, capture_lasers
from .forward_project import forward_project
from .loss import loss as fused_loss
from .train import (Adam, OptimizationParams, TrainStep, add_mcmc_arguments, check_mcmc_arguments, mcmc_options,
                    run_steps)
from .voxelize import VoxelGrid, front_view, voxelize, voxelize_backward

SH_C0 = 0.28209479177387814


class VoxelFitStep:
    """One fused fit iteration per call (see the module docstring); returns the device [2] loss of the step
    ((MSE, equal_loss), or (mean deviance, deviance per count) with loss="poisson").

    model          GaussianModel-like (raw tensors under the reference's names), updated in place.
    grid, cam      the VoxelGrid and the albedo view point [3] of voxelize; preset, cutoff, scaling_modifier as there.
    target_volume  [nx, ny, nz]: volume mode.  Exactly one of target_volume and rows is given.
    rows, walls, r0, dr, power, lasers   capture mode: rows [nwall, nr] measured at walls [nwall, 3], window and
                   weight as forward_project takes them (power 0..4), lasers as there (None: confocal).
    rows, operator capture mode through the LCT operator pair: an nlosgr.lct.LctOperator in place of walls=, r0=,
                   dr=, power= and lasers= (it carries them; passing both raises).  grid must have the operator's
                   volume shape (W, nr, H) (operator.grid); project is operator.forward, the gradient operator.adjoint.
    irf, loss, rate_floor, gt_times      the fused loss's, as in TrainStep (capture mode only).
    volume_scale   the factor between A(albedo_density) and the rows' units (voxel volume, bin width, gain).
    keep_grads     keep the last step's gradients in self.grads (train.GROUPS order), its volume in self.volume,
                   the projected rows in self.rows_pred and dL/dvolume in self.grad_volume."""

    def __init__(self, model, grid, cam, preset="cuda", cutoff=3.0, scaling_modifier=1.0, target_volume=None,
                 rows=None, walls=None, r0=None, dr=None, power=0, lasers=None, irf=None, loss="mse", rate_floor=1.0,
                 gt_times=1.0, volume_scale=1.0, opt=None, spatial_lr_scale=1.0, keep_grads=False, sh_schedule=False,
                 operator=None):
        if not isinstance(grid, VoxelGrid):
            raise TypeError("nlosgr: grid must be a voxelize.VoxelGrid")
        if (target_volume is None) == (rows is None):
            raise ValueError("nlosgr: VoxelFitStep takes exactly one target: target_volume= (volume mode) or rows= "
                             "with walls=, r0=, dr= (capture mode)" + ("; both were given" if rows is not None
                                                                         else "; none was given"))
        if operator is not None:
            from .lct import LctOperator
            if not isinstance(operator, LctOperator):
                raise TypeError("nlosgr: operator= must be an nlosgr.lct.LctOperator")
            if rows is None:
                raise ValueError("nlosgr: operator= belongs to rows= (capture mode), not to target_volume=")
            if walls is not None or lasers is not None or r0 is not None or dr is not None:
                raise ValueError("nlosgr: operator= carries the lattice, the window and the power: it cannot be combined "
                                 "with walls=, lasers=, r0= or dr=")
            if grid.shape != operator.volume_shape:
                raise ValueError(f"nlosgr: with operator= the grid must have the operator's volume shape "
                                 f"{operator.volume_shape} (operator.grid), got {grid.shape}")
        if rows is not None and not 0 <= int(power) <= 4:
            raise ValueError("nlosgr: VoxelFitStep takes a power in 0..4 (the range of backproject, the projector's "
                             f"adjoint), got {int(power)}; scale the rows by r^q for the falloff (fit_capture falloff=)")
        if preset not in _lib.PRESETS:
            raise ValueError(f"nlosgr: preset must be one of {tuple(_lib.PRESETS)}")
        if loss not in _lib.LOSSES:
            raise ValueError(f"nlosgr: loss must be one of {tuple(_lib.LOSSES)}, got {loss!r}")
        self.model, self.grid = model, grid
        self.preset, self.cutoff, self.scaling_modifier = preset, float(cutoff), float(scaling_modifier)
        self.loss_kind, self.rate_floor, self.gt_times = loss, float(rate_floor), float(gt_times)
        self.volume_scale = float(volume_scale)
        dev = model._mu.device
        self.cam = torch.as_tensor(cam, dtype=torch.float32).reshape(-1).to(dev).contiguous()
        if self.cam.numel() != 3:
            raise ValueError("nlosgr: cam must have 3 elements")
        self.target_volume = self.rows = self.walls = self.lasers = self.operator = None
        if target_volume is not None:
            if irf is not None or loss != "mse":
                raise ValueError("nlosgr: volume mode is the MSE against the volume: irf= and loss= belong to rows=")
            self.target_volume = _gpu_f32(target_volume, "VoxelFitStep")
            if tuple(self.target_volume.shape) != grid.shape:
                raise ValueError(f"nlosgr: target_volume must have the grid's shape {grid.shape}")
        elif operator is not None:
            self.rows, self.operator = _gpu_f32(rows, "VoxelFitStep"), operator
            if tuple(self.rows.shape) != operator.rows_shape or self.rows.device != operator.device:
                raise ValueError(f"nlosgr: with operator= the rows must be {operator.rows_shape} on {operator.device}")
        else:
            if walls is None or r0 is None or dr is None:
                raise ValueError("nlosgr: capture mode needs walls=, r0= and dr= with rows=")
            self.rows, self.walls = _gpu_f32(rows, "VoxelFitStep"), _gpu_f32(walls, "VoxelFitStep")
            if (self.rows.dim() != 2 or self.walls.dim() != 2 or self.walls.shape[1] != 3
                    or self.walls.shape[0] != self.rows.shape[0]):
                raise ValueError("nlosgr: VoxelFitStep takes rows [nwall, nr] and walls [nwall, 3]")
            if not float(dr) > 0:
                raise ValueError("nlosgr: dr must be > 0")
            self.r0, self.dr, self.power = float(r0), float(dr), int(power)
            self.lasers = _lasers_arg(lasers, self.walls, "VoxelFitStep") if lasers is not None else None
        self.irf = irf.to(dev) if irf is not None else None
        self.opt = opt or OptimizationParams()
        self.spatial_lr_scale = float(spatial_lr_scale)
        self.keep_grads, self.sh_schedule = keep_grads, sh_schedule
        self.grads = self.volume = self.rows_pred = self.grad_volume = None
        self.iteration = 0
        self._occl_plan = None
        ng = model._mu.shape[0]
        self._tensors = [model._mu.data, model._features_dc.data.view(ng, -1), model._features_rest.data.view(ng, -1),
                         model._opacity.data.view(ng), model._scaling.data, model._rotation.data]
        self.adam = Adam(self._tensors, eps=1e-15)

    # TrainStep's own: the schedule, the density-control hook, and regulariser + keep_grads + Adam + SH schedule
    learning_rates = TrainStep.learning_rates
    rebind = TrainStep.rebind
    _activation = TrainStep._activation
    _finish = TrainStep._finish

    def project(self, volume):
        """volume_scale * A_power(volume): the rows the loss compares with the capture (capture mode)."""
        if self.operator is not None:
            rows = self.operator.forward(volume)
        else:
            rows = forward_project(volume, self.walls, self.grid, self.r0, self.dr, self.rows.shape[1],
                                   power=self.power, lasers=self.lasers)
        return rows if self.volume_scale == 1.0 else rows.mul_(self.volume_scale)

    @torch.no_grad()
    def __call__(self, iteration=None):
        it = self.iteration if iteration is None else iteration
        m = self.model
        kw = dict(preset=self.preset, cutoff=self.cutoff, scaling_modifier=self.scaling_modifier)
        _, vol = voxelize(m, self.grid, self.cam, want_density=False, **kw)
        rows_pred = None
        if self.target_volume is not None:
            loss2, g_vol = fused_loss(vol, self.target_volume, 1.0)
        else:
            rows_pred = self.project(vol)
            loss2, g_rows = fused_loss(rows_pred, self.rows, self.gt_times, irf=self.irf, kind=self.loss_kind,
                                       rate_floor=self.rate_floor)
            if self.operator is not None:
                g_vol = self.operator.adjoint(g_rows)
            else:
                g_vol = backproject(g_rows, self.walls, self.grid, self.r0, self.dr, power=self.power,
                                    lasers=self.lasers)
            if self.volume_scale != 1.0:
                g_vol.mul_(self.volume_scale)
        if self.keep_grads:
            self.volume, self.rows_pred, self.grad_volume = vol, rows_pred, g_vol
        d_mu, d_s, d_q, d_o, d_f = voxelize_backward(m, self.grid, self.cam, None, g_vol, **kw)
        return self._finish([d_mu, d_f[:, :1], d_f[:, 1:], d_o, d_s, d_q], loss2, it)


def fit_capture(data_kwargs, model, resolution, start, end, power=0, falloff=0, cam=None, projector="exact", nv=None,
                **kw):
    """The VoxelFitStep of a loaded capture (data.make_data_kwargs), laid out as landweber_capture lays it out:
    bins [floor(start), floor(start) + end - start) of every measurement against VoxelGrid(volume_position,
    volume_size, resolution), r0 = floor(start) c deltaT, dr = c deltaT, the capture's laser spots when it is
    non-confocal and its IRF when it has one.  cam defaults to the volume position projected onto the wall.
    falloff=q multiplies bin j of the rows by (r0 + j dr)^q first, the compensation the operator's power cannot
    give (it has no negative power).  For a non-confocal capture this compensates the physical (dl ds)^-2 only
    approximately: the bin fixes g = (dl + ds) / 2, and dl ds <= g^2 with equality only where dl = ds; landweber
    on such a capture has the same limitation.  Further keywords go to VoxelFitStep.
    projector="lct": through the LCT operator pair instead (VoxelFitStep(operator=)): a confocal capture on a wall
    lattice (lct.lct_capture's errors otherwise), the grid is the lattice's own fk.fk_grid, uncropped, so resolution
    is not used; power may be -4..4, nv is the operator's cell count; falloff works as above."""
    if projector not in ("exact", "lct"):
        raise ValueError("nlosgr: projector must be 'exact' or 'lct'")
    if projector == "lct":
        from .lattice import confocal_lattice
        from .lct import LctOperator
        c = confocal_lattice(data_kwargs, start, end, "the LCT projector")
        rows = _gpu_f32(c.rows.float(), "fit_capture")
        if falloff:
            radii = c.r0 + c.dr * torch.arange(c.nr, dtype=torch.float64, device=rows.device)
            rows = (rows.double() * radii.pow(float(falloff))[None]).float()
        op = LctOperator(c.H, c.W, c.sx, c.sz, c.r0, c.dr, c.nr, power=power, nv=nv, perm=c.perm, x_along=c.x_along,
                         device=rows.device)
        if cam is None:
            cam = (float(data_kwargs["volume_position"][0]), 0.0, float(data_kwargs["volume_position"][2]))
        kw.setdefault("irf", data_kwargs.get("irf"))
        return VoxelFitStep(model, op.grid(c.xs, c.zs, c.y0), cam, rows=rows, operator=op, **kw)
    from .data import volume_target
    I1 = int(np.floor(start))
    nr = int(end - start)
    rows = _gpu_f32(volume_target(data_kwargs, start, nr), "fit_capture")
    cdt = float(data_kwargs["c"]) * float(data_kwargs["deltaT"])
    r0 = I1 * cdt
    if falloff:
        radii = r0 + cdt * torch.arange(nr, dtype=torch.float64, device=rows.device)
        rows = (rows.double() * radii.pow(float(falloff))[None]).float()
    walls = data_kwargs["camera_grid_positions"].t().contiguous().float()
    vp = [float(v) for v in data_kwargs["volume_position"]]
    grid = VoxelGrid(vp, float(data_kwargs["volume_size"]), resolution)
    if cam is None:
        cam = (vp[0], 0.0, vp[2])
    kw.setdefault("irf", data_kwargs.get("irf"))
    return VoxelFitStep(model, grid, cam, rows=rows, walls=walls, r0=r0, dr=cdt, power=power,
                        lasers=capture_lasers(data_kwargs), **kw)


def model_from_points(points, rho, spacing, sh_degree=1):
    """GaussianParams (cuda preset) at points [n, 3] with albedo rho [n, 1]: isotropic, std = spacing, identity
    rotation, opacity 0 (sigma = 1/2), dc = (rho - 1/2) / C0 as the reference's RHO2SH, higher SH zero (degree >= 1:
    the step's Adam groups are views of non-empty tensors)."""
    from .model import GaussianParams
    pts = torch.as_tensor(points).float()
    dev, n = pts.device, pts.shape[0]
    K = (int(sh_degree) + 1) ** 2
    rho = torch.as_tensor(np.asarray(rho), dtype=torch.float32, device=dev).reshape(n, 1, 1)
    rot = torch.zeros(n, 4, device=dev)
    rot[:, 0] = 1.0
    return GaussianParams(pts.contiguous(), torch.full((n, 3), math.log(float(spacing)), device=dev), rot,
                          torch.zeros(n, 1, device=dev), (rho - 0.5) / SH_C0, torch.zeros(n, K - 1, 1, device=dev),
                          sh_degree, sh_degree)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nlosgr.voxel_fit",
                                 description="Fit Gaussians to a confocal or non-confocal capture (the optional field "
                                             "laserGridPositions) through the voxel grid: voxelize, forward-project, "
                                             "loss, back-project, voxelizer backward, Adam.")
    ap.add_argument("capture", help="Zaragoza-format .mat file")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--start", type=int, required=True, help="first time bin")
    ap.add_argument("--end", type=int, required=True, help="one past the last time bin")
    ap.add_argument("--gaussians", type=int, required=True, help="number of Gaussians")
    ap.add_argument("--iterations", type=int, required=True)
    ap.add_argument("--power", type=int, default=0, choices=range(-4, 5),
                    help="weight d^power of the operator: 0..4 (--projector lct: -4..4)")
    # (absent from the namespace unless given: a run without them parses to what it did before they existed)
    ap.add_argument("--projector", choices=("exact", "lct"), default=argparse.SUPPRESS,
                    help="exact (default): every (voxel, wall point) pair on a --resolution grid; lct: the LCT operator "
                         "pair on the wall lattice's own voxels (a confocal capture on a lattice)")
    ap.add_argument("--nv", type=int, default=argparse.SUPPRESS,
                    help="--projector lct: depth-squared cells (default: the bins)")
    ap.add_argument("--falloff", type=float, default=0.0, help="multiply bin j of the rows by (r0 + j dr)^falloff")
    ap.add_argument("--cutoff", type=float, default=3.0, help="Mahalanobis support radius; <= 0: dense")
    ap.add_argument("--loss", choices=sorted(_lib.LOSSES), default="mse")
    ap.add_argument("--out", required=True, help="checkpoint to write")
    add_mcmc_arguments(ap)
    ap.add_argument("--recon", default=None, help="also write the fitted Gaussians' voxel volume (nlosgr.voxelize keys)")
    a = ap.parse_args(argv)
    if a.end <= a.start:
        ap.error("--end must be greater than --start")
    if a.iterations < 1:
        ap.error("--iterations must be >= 1")
    check_mcmc_arguments(ap, a)
    if a.gaussians < 1:
        ap.error("--gaussians must be >= 1")
    if a.resolution < 2:
        ap.error("--resolution must be >= 2")
    if getattr(a, "projector", "exact") == "exact" and a.power < 0:
        ap.error("--power must be in 0..4 with --projector exact")
    if getattr(a, "projector", "exact") == "exact" and hasattr(a, "nv"):
        ap.error("--nv belongs to --projector lct")
    return a


def main(argv=None):
    a = parse_args(argv)
    from types import SimpleNamespace

    from .checkpoint import save_checkpoint
    from .data import make_data_kwargs
    from .init import sample_from_backprojection
    if not torch.cuda.is_available():
        raise RuntimeError("nlosgr: voxel_fit needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    dk, *_ = make_data_kwargs(a.capture, dev, shuffle=False)
    init = SimpleNamespace(init_gaussian_num=a.gaussians, carving_volume_size=a.resolution, start=a.start, end=a.end)
    pts, rho = sample_from_backprojection(init, dk)
    spacing = float(dk["volume_size"]) / (a.resolution - 1)
    model = model_from_points(pts, rho, spacing)
    step = fit_capture(dk, model, a.resolution, a.start, a.end, power=a.power, falloff=a.falloff, preset="cuda",
                       cutoff=a.cutoff, loss=a.loss, opt=mcmc_options(a), projector=getattr(a, "projector", "exact"),
                       nv=getattr(a, "nv", None))
    # one least-squares gain between A(albedo_density) and the rows, from the initial Gaussians (one host read)
    pred = step.project(voxelize(model, step.grid, step.cam, preset="cuda", cutoff=a.cutoff, want_density=False)[1])
    den = float(pred.double().square().sum())
    if den > 0:
        step.volume_scale = float((pred.double() * step.rows.double()).sum()) / den
    losses = run_steps(step, a).cpu().numpy()
    save_checkpoint(a.out, model, train_step=step)
    print(f"wrote {a.out}: {model._mu.shape[0]} Gaussians, {step.grid.shape} voxels, bins [{a.start}, {a.end}), power "
          f"{a.power}, falloff {a.falloff:g}, {a.iterations} iterations, loss {losses[0]:.6g} -> {losses[-1]:.6g}")
    if a.recon:
        dens, alb = voxelize(model, step.grid, step.cam, preset="cuda", cutoff=a.cutoff)
        front, depth = front_view(alb, step.grid)
        grid = step.grid
        np.savez_compressed(a.recon, density=dens.cpu().numpy(), albedo=alb.cpu().numpy(), front=front.cpu().numpy(),
                            depth=depth.cpu().numpy(), xs=grid.xs.numpy(), ys=grid.ys.numpy(), zs=grid.zs.numpy(),
                            cam=step.cam.cpu().numpy())
        print(f"wrote {a.recon}")


if __name__ == "__main__":
    main()
