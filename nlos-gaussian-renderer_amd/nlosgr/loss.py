"""Photon-count likelihood: the loss of a measured capture.

A measured transient is a histogram of photon counts.  Its noise is Poisson: the variance of a bin is its
rate.  The MSE is the likelihood of constant-variance Gaussian noise; on a capture it puts nearly all its
weight on the bright first-return peak and treats the low-count tail and the dark floor as exact.  The
Poisson deviance weighs every bin by its own noise.  Per element, with t the target, gt = gt_times,
lambda the model rate (the render through the IRF, its background included) and eps = rate_floor > 0:

    y'  = max(gt t, 0) + eps          measured counts plus the floor
    rho = max(lambda, 0) + eps        model rate plus the same floor
    dev = 2 [y' log(y'/rho) - (y' - rho)]  =  2 y' (e - log1p(e)),   e = (rho - y') / y'
    dL/dlambda ~ (rho - y') / rho   where lambda >= 0,   0 where lambda < 0

dev >= 0, and 0 exactly when rho = y'; empty bins need no special case (y' >= eps > 0).  With non-negative
taps, render and background the clamp on lambda never acts.

rate_floor: the target times gt_times is meant to be in counts, and gt_times is the knob that brings a
capture there.  The capture's dark-count level is the natural value of the floor; the default, one
pseudo-count, keeps the gradient factor (rho - y') / rho of a bin the render does not reach yet at about
-y instead of -y / eps.

    loss              the fused loss of a kind ("mse" or "poisson") on the GPU (nlosgr_loss_irf)
    PoissonDeviance   the same mean deviance in plain torch, differentiable: a criterion for compute_loss
    simulate_capture  a render (through an IRF) -> Poisson counts, a noisy synthetic capture
"""
import ctypes
import math

import torch

from . import _lib
from .irf import IRF, convolve_time

KINDS = tuple(_lib.LOSSES)

_identity = {}   # device -> the one-tap identity IRF (w = {1}, c = 0, b = 0)


def identity_irf(device):
    """The cached identity IRF on `device`."""
    device = torch.device(device)
    if device not in _identity:
        _identity[device] = IRF(torch.ones(1, dtype=torch.float32, device=device), 0, 0.0)
    return _identity[device]


def _check_floor(rate_floor):
    rate_floor = float(rate_floor)
    if not (math.isfinite(rate_floor) and rate_floor > 0.0):
        raise ValueError("nlosgr: rate_floor must be finite and > 0")
    return rate_floor


def loss(hist, target, gt_times=1.0, grad_scale=1.0, want_grad=True, raw=False, irf=None, kind="mse", rate_floor=1.0):
    """(loss2, grad) of the fused loss, with the return convention of nlosgr.train.mse.

    kind="mse": nlosgr.train.mse, unchanged (nlosgr_mse without an IRF, nlosgr_mse_irf with one); rate_floor
    is ignored.
    kind="poisson": loss2 = device [2] = (mean deviance, deviance per measured count) against gt_times *
    target, grad = grad_scale * d(mean deviance)/dhist; raw=True returns the device [4] (those two, sum dev,
    sum max(gt target, 0)), whose [2:4] combine over bands and batches as the MSE's raw sums do.  Without an
    IRF the identity IRF is used, so the time axis is at most 8192 bins either way."""
    if kind not in _lib.LOSSES:
        raise ValueError(f"nlosgr: loss kind must be one of {KINDS}, got {kind!r}")
    if kind == "mse":
        from .train import mse
        return mse(hist, target, gt_times, grad_scale, want_grad, raw, irf)
    rate_floor = _check_floor(rate_floor)
    lib = _lib.load()
    dev = hist.device
    h = hist.detach().contiguous()
    t = target.detach().contiguous()
    if h.shape != t.shape or h.dtype != torch.float32 or t.dtype != torch.float32:
        raise ValueError("nlosgr: hist and target must be float32 tensors of one shape")
    if h.dim() < 1:
        raise ValueError("nlosgr: the photon-count loss needs a time axis")
    nr = h.shape[-1]
    rows = h.numel() // nr if nr else 0
    irf = identity_irf(dev) if irf is None else irf.to(dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    grad = torch.empty_like(h) if want_grad else None
    s = irf.struct()
    spec = _lib.Loss(_lib.LOSSES[kind], rate_floor)
    ws = torch.empty(lib.nlosgr_loss_irf_workspace_bytes(rows) // 4, dtype=torch.float32, device=dev)
    _lib.check(lib.nlosgr_loss_irf(_lib.ptr(h), _lib.ptr(t), float(gt_times), rows, nr, ctypes.byref(s),
                                   ctypes.byref(spec), float(grad_scale), _lib.ptr(grad), _lib.ptr(ws), _lib.ptr(out),
                                   _lib.stream_handle(dev)))
    return (out if raw else out[:2]), grad


class PoissonDeviance:
    """criterion(pred, target) -> the mean Poisson deviance, in plain torch (CPU or GPU, any float dtype,
    differentiable in pred).  target is in counts (compute_loss has multiplied gt_times in); pred is the
    model rate.  It slots into optim_kwargs["criterion"] of nlos_helpers.compute_loss, where the prediction
    has already passed through data_kwargs["irf"], and it is the composition the fused step is tested against."""

    def __init__(self, rate_floor=1.0):
        self.rate_floor = _check_floor(rate_floor)

    def __call__(self, pred, target):
        eps = self.rate_floor
        yp = target.detach().clamp_min(0) + eps
        rho = pred.clamp_min(0) + eps
        e = (rho - yp) / yp
        return (2.0 * yp * (e - torch.log1p(e))).mean()

    def __repr__(self):
        return f"PoissonDeviance(rate_floor={self.rate_floor})"


def simulate_capture(hist, irf=None, photons=None, generator=None):
    """(counts, scale): a noisy synthetic capture of a rendered transient.  rate = max(convolve_time(hist, irf), 0)
    (hist itself without an IRF; the IRF's background is part of the rate); with `photons` the rate is scaled to
    sum to that many expected counts (scale = photons / sum rate, else 1); counts = Poisson(rate) as float32, of
    hist's shape.  CPU or GPU tensors; torch's sampler (`generator` seeds it).  With data.save_zaragoza(..., irf=)
    this writes a capture file to train against."""
    with torch.no_grad():
        h = hist.detach()
        rate = (convolve_time(h, irf) if irf is not None else h).clamp_min(0)
        scale = 1.0
        if photons is not None:
            total = rate.double().sum().item()
            scale = float(photons) / total if total > 0 else 1.0
            rate = (rate.double() * scale).to(rate.dtype)
        counts = torch.poisson(rate, generator=generator).to(torch.float32)
    return counts, scale
