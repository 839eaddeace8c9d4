"""The Gaussian renderer of a non-confocal capture (laser spot != sensed point): nlosgr_render_nc_fwd / _bwd.

    hist [nmeas, nr] = hscale[p] att[k] sum_ij sin(theta_i) q_pijk sum_g w_g(p) pdf_g(x_pijk)

with x the point of ray ij of the sensed point s_p on the ellipsoid |x - s_p| + |x - l_p| = 2 r[k] and q the ratio of
the exact shell measure and falloff to the confocal ones (include/nlosgr.h states the formulas and the contract).
`geo` is the Geometry of the SENSED points (data.volume_geometry_nc, or geometry.build_geometry), `lasers` is
[nmeas, 3] (one spot per measurement), [1, 3] (one spot for the capture) or the capture file's [3, n] layout.
With lasers == sensors this is the confocal renderer's quantity (another kernel, another summation order).

render_nc_forward / render_nc_backward are the plain calls, render_nc the autograd front (as render.render), and
NcTrainStep one fused training iteration per call: render -> fused loss (MSE or Poisson deviance through the IRF)
-> backward -> nlosgr_adam, built like voxel_fit.VoxelFitStep, so densify.relocate_gs / add_new_gs(train_step=)
and checkpoint.save_checkpoint(train_step=) take it as they take a TrainStep.

Scope: the no-occlusion histogram under support selection (cfg.mode "noocl", cfg.selection "support"); no per-ray
output and no ray cache (cfg.ray_cache is ignored).  Sharding needs no code of its own: a row of the result depends
on its measurement alone, so geo.slice / geo.rows with the same rows of `lasers` render bitwise those rows, and the
gradients of the shards add.

    python -m nlosgr.render_nc CAPTURE.mat --start S --end E --ns N --gaussians G --iterations I [--cutoff C]
        --out CKPT
"""
import argparse
from dataclasses import replace

import torch

from . import _lib
from .backproject import _lasers_arg
from .loss import loss as fused_loss
from .render import RenderConfig, _as_f32, _structs
from .train import (Adam, OptimizationParams, TrainStep, add_mcmc_arguments, check_mcmc_arguments, mcmc_options,
                    run_steps)


def lasers_for(lasers, geo, what="render_nc"):
    """lasers as the entry points take them: float32 [nmeas, 3] or [1, 3] on the geometry's device.  The capture
    file's [3, n] layout (data_kwargs["laser_grid_positions"]) is transposed; a square [3, 3] is read as [n, 3]."""
    if not isinstance(lasers, torch.Tensor):
        raise TypeError(f"nlosgr: {what} takes lasers as a tensor")
    if lasers.dim() == 2 and lasers.shape[0] == 3 and lasers.shape[1] != 3:
        lasers = lasers.t()
    return _lasers_arg(lasers.float(), geo.wall, what)


def _nc_structs(mu, scaling, rotation, opacity, features, geo, cfg):
    if cfg.mode != "noocl" or cfg.selection != "support":
        raise ValueError("nlosgr: the non-confocal renderer serves mode='noocl' with selection='support' only "
                         f"(got mode={cfg.mode!r}, selection={cfg.selection!r})")
    return _structs(mu, scaling, rotation, opacity, features, geo, cfg, False)


def _workspace(lib, g, gs, nlaser, o, device):
    nbytes = lib.nlosgr_render_nc_workspace_bytes(g, gs, nlaser, o)
    if nbytes == 0:
        _lib.check(1)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


@torch.no_grad()
def render_nc_forward(mu, scaling, rotation, opacity, features, geo, lasers, cfg):
    """hist [nmeas, nr] (not differentiable)."""
    lib = _lib.load()
    dev = mu.device
    mu, scaling, rotation, opacity, features = [_as_f32(t) for t in (mu, scaling, rotation, opacity, features)]
    lasers = lasers_for(lasers, geo, "render_nc_forward")
    g, gs, o = _nc_structs(mu, scaling, rotation, opacity, features, geo, cfg)
    ws = _workspace(lib, g, gs, lasers.shape[0], o, dev)
    hist = torch.empty(geo.nwall, geo.nr, device=dev)
    _lib.check(lib.nlosgr_render_nc_fwd(g, gs, _lib.ptr(lasers), lasers.shape[0], o, _lib.ptr(ws), _lib.ptr(hist),
                                        _lib.stream_handle(dev)))
    return hist


@torch.no_grad()
def render_nc_backward(mu, scaling, rotation, opacity, features, geo, lasers, cfg, grad_hist):
    """(d_mu, d_scaling, d_rotation, d_opacity [ng], d_features [ng, K]) of sum(hist grad_hist)."""
    lib = _lib.load()
    dev = mu.device
    mu, scaling, rotation, opacity, features = [_as_f32(t) for t in (mu, scaling, rotation, opacity, features)]
    lasers = lasers_for(lasers, geo, "render_nc_backward")
    g, gs, o = _nc_structs(mu, scaling, rotation, opacity, features, geo, cfg)
    ws = _workspace(lib, g, gs, lasers.shape[0], o, dev)
    gh = _as_f32(grad_hist)
    if tuple(gh.shape) != (geo.nwall, geo.nr):
        raise ValueError(f"nlosgr: grad_hist must be [{geo.nwall}, {geo.nr}]")
    d_mu, d_s, d_q = torch.empty_like(mu), torch.empty_like(scaling), torch.empty_like(rotation)
    d_o, d_f = torch.empty(mu.shape[0], device=dev), torch.empty_like(features)
    _lib.check(lib.nlosgr_render_nc_bwd(g, gs, _lib.ptr(lasers), lasers.shape[0], o, _lib.ptr(ws), _lib.ptr(gh),
                                        _lib.ptr(d_mu), _lib.ptr(d_s), _lib.ptr(d_q), _lib.ptr(d_o), _lib.ptr(d_f),
                                        _lib.stream_handle(dev)))
    return d_mu, d_s, d_q, d_o, d_f


class RenderNcFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, scaling, rotation, opacity, features, geo, lasers, cfg):
        hist = render_nc_forward(mu, scaling, rotation, opacity, features, geo, lasers, cfg)
        ctx.save_for_backward(mu, scaling, rotation, opacity, features)
        ctx.geo, ctx.lasers, ctx.cfg, ctx.oshape = geo, lasers, cfg, opacity.shape
        return hist

    @staticmethod
    def backward(ctx, g_hist):
        mu, scaling, rotation, opacity, features = ctx.saved_tensors
        d_mu, d_s, d_q, d_o, d_f = render_nc_backward(mu, scaling, rotation, opacity, features, ctx.geo, ctx.lasers,
                                                      ctx.cfg, g_hist.float().contiguous())
        return d_mu, d_s, d_q, d_o.reshape(ctx.oshape), d_f, None, None, None


def render_nc(mu, scaling, rotation, opacity, features, geo, lasers, cfg):
    """Differentiable non-confocal render: hist [nmeas, nr]."""
    return RenderNcFn.apply(mu, scaling, rotation, opacity, features, geo, lasers, cfg)


class NcTrainStep:
    """One fused training iteration on a non-confocal capture per call; returns the device [2] loss of the step
    ((MSE, equal_loss), or (mean deviance, deviance per count) with loss="poisson").

    model    GaussianModel-like (raw tensors under the reference's names), updated in place.
    geo      Geometry of the sensed points; lasers as render_nc_forward takes them.
    cfg      render.RenderConfig (mode "noocl", selection "support"); its sh_degree follows the model's.
    target   [nmeas, nr] measured histograms (before gt_times); irf, loss, rate_floor, gt_times as TrainStep.
    keep_grads   keep the last step's gradients in self.grads (train.GROUPS order), its render in self.hist and
                 dL/dhist in self.grad_hist.
    A shard of the capture is geo.slice / geo.rows with the same rows of lasers and target; this step is
    single-process (the gradients of shards add, the loss sums are loss(raw=True)'s)."""

    def __init__(self, model, geo, lasers, cfg, target, gt_times=1.0, irf=None, loss="mse", rate_floor=1.0, opt=None,
                 spatial_lr_scale=1.0, keep_grads=False, sh_schedule=False):
        if loss not in _lib.LOSSES:
            raise ValueError(f"nlosgr: loss must be one of {tuple(_lib.LOSSES)}, got {loss!r}")
        if cfg.mode != "noocl" or cfg.selection != "support":
            raise ValueError("nlosgr: NcTrainStep takes mode='noocl' with selection='support'")
        self.model, self.geo, self.cfg = model, geo, cfg
        self.lasers = lasers_for(lasers, geo, "NcTrainStep")
        self.target = target.detach().float().contiguous()
        if tuple(self.target.shape) != (geo.nwall, geo.nr):
            raise ValueError(f"nlosgr: target must be [{geo.nwall}, {geo.nr}]")
        self.loss_kind, self.rate_floor, self.gt_times = loss, float(rate_floor), float(gt_times)
        dev = model._mu.device
        self.irf = irf.to(dev) if irf is not None else None
        self.opt = opt or OptimizationParams()
        self.spatial_lr_scale = float(spatial_lr_scale)
        self.keep_grads, self.sh_schedule = keep_grads, sh_schedule
        self.grads = self.hist = self.grad_hist = None
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

    @torch.no_grad()
    def __call__(self, iteration=None):
        from . import features_flat
        it = self.iteration if iteration is None else iteration
        m = self.model
        cfg = replace(self.cfg, sh_degree=int(m.active_sh_degree))
        args = (m._mu.detach(), m._scaling.detach(), m._rotation.detach(), m._opacity.detach(),
                features_flat(m).detach().contiguous(), self.geo, self.lasers, cfg)
        hist = render_nc_forward(*args)
        loss4, grad = fused_loss(hist, self.target, self.gt_times, raw=True, irf=self.irf, kind=self.loss_kind,
                                 rate_floor=self.rate_floor)
        if self.keep_grads:
            self.hist, self.grad_hist = hist, grad
        d_mu, d_s, d_q, d_o, d_f = render_nc_backward(*args, grad)
        return self._finish([d_mu, d_f[:, :1], d_f[:, 1:], d_o, d_s, d_q], loss4[:2], it)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nlosgr.render_nc",
                                 description="Fit Gaussians to a confocal or non-confocal capture (the optional field "
                                             "laserGridPositions) with the non-confocal Gaussian renderer: render, "
                                             "fused loss, backward, Adam.")
    ap.add_argument("capture", help="Zaragoza-format .mat file")
    ap.add_argument("--start", type=int, required=True, help="first time bin")
    ap.add_argument("--end", type=int, required=True, help="one past the last time bin")
    ap.add_argument("--ns", type=int, default=32, help="theta and phi samples per sensed point")
    ap.add_argument("--gaussians", type=int, required=True, help="number of Gaussians")
    ap.add_argument("--iterations", type=int, required=True)
    ap.add_argument("--cutoff", type=float, default=5.7, help="Mahalanobis support radius; <= 0: dense")
    ap.add_argument("--resolution", type=int, default=64, help="grid of the back-projection the Gaussians start from")
    ap.add_argument("--loss", choices=sorted(_lib.LOSSES), default="mse")
    ap.add_argument("--out", required=True, help="checkpoint to write")
    add_mcmc_arguments(ap)
    a = ap.parse_args(argv)
    if a.end <= a.start:
        ap.error("--end must be greater than --start")
    if a.iterations < 1:
        ap.error("--iterations must be >= 1")
    check_mcmc_arguments(ap, a)
    if a.gaussians < 1:
        ap.error("--gaussians must be >= 1")
    if a.ns < 1:
        ap.error("--ns must be >= 1")
    if a.resolution < 2:
        ap.error("--resolution must be >= 2")
    return a


def main(argv=None):
    a = parse_args(argv)
    from types import SimpleNamespace

    from .checkpoint import save_checkpoint
    from .data import make_data_kwargs, volume_geometry_nc, volume_target
    from .init import sample_from_backprojection
    from .voxel_fit import model_from_points
    if not torch.cuda.is_available():
        raise RuntimeError("nlosgr: render_nc needs a GPU (no CPU fallback)")
    dev = torch.device("cuda:0")
    dk, *_ = make_data_kwargs(a.capture, dev, shuffle=False)
    init = SimpleNamespace(init_gaussian_num=a.gaussians, carving_volume_size=a.resolution, start=a.start, end=a.end)
    pts, rho = sample_from_backprojection(init, dk)
    model = model_from_points(pts, rho, float(dk["volume_size"]) / (a.resolution - 1))
    geo, lasers = volume_geometry_nc(dk, a.ns, a.start, a.end, preset="cuda")
    target = volume_target(dk, a.start, geo.nr)
    cfg = RenderConfig(preset="cuda", mode="noocl", cutoff=a.cutoff, c_deltaT=float(dk["c"]) * float(dk["deltaT"]))
    step = NcTrainStep(model, geo, lasers, cfg, target, irf=dk.get("irf"), loss=a.loss, opt=mcmc_options(a))
    # one least-squares gain between the initial render and the capture (one host read)
    from . import features_flat
    pred = render_nc_forward(model._mu, model._scaling, model._rotation, model._opacity, features_flat(model), geo,
                             lasers, replace(cfg, sh_degree=int(model.active_sh_degree)))
    den = float(target.double().square().sum())
    num = float((pred.double() * target.double()).sum())
    if den > 0 and num > 0:
        step.gt_times = num / den
    losses = run_steps(step, a).cpu().numpy()
    save_checkpoint(a.out, model, train_step=step)
    print(f"wrote {a.out}: {model._mu.shape[0]} Gaussians, {geo.nwall} measurements x {geo.nr} bins [{a.start}, {a.end}), "
          f"{a.ns} x {a.ns} rays, cutoff {a.cutoff:g}, {a.iterations} iterations, loss {losses[0]:.6g} -> "
          f"{losses[-1]:.6g}")


if __name__ == "__main__":
    main()
