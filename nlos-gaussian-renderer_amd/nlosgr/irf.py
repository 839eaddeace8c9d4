"""Temporal instrument response: the step between a rendered transient and a measured one.

A capture is the ideal transient convolved in time with the system's impulse response (laser pulse
width (*) detector jitter, often with a diffusion tail) on a constant floor of dark counts and
ambient light.  Rows are wall points and the time axis is last.  An IRF is L real taps w, a centre
c (0 <= c < L) and a background b (include/nlosgr.h, ABI 12):

    apply:    y[p,t] = b + sum_j w[j] h[p, t + c - j]      (h = 0 outside [0, nr))
    adjoint:  g[p,s] =     sum_j w[j] z[p, s - c + j]      (z = 0 outside [0, nr))

c = 0 is a causal response; c = argmax w keeps a peak where it was.  Taps may be negative and are
not normalised here (IRF.normalized() does).  Light from before the rendered window [start, end)
counts as zero: render a window widened by the IRF's length where the early bins matter.

The IRF is a property of the capture, not of the model: checkpoints do not store it
(nlosgr.data.load_irf reads it from the capture file).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

MAX_TAPS = 512   # NLOSGR_IRF_MAX_TAPS


class IRF:
    """taps: 1-D tensor / array (kept as float32); center=None -> argmax of the taps."""

    def __init__(self, taps, center=None, background=0.0):
        t = taps.detach() if torch.is_tensor(taps) else torch.as_tensor(np.asarray(taps, dtype=np.float64))
        if t.dim() != 1:
            raise ValueError("nlosgr: IRF taps must be one-dimensional")
        L = t.numel()
        if not 1 <= L <= MAX_TAPS:
            raise ValueError(f"nlosgr: an IRF has 1..{MAX_TAPS} taps, got {L}")
        if center is None:
            center = int(torch.argmax(t))
        center = int(center)
        if not 0 <= center < L:
            raise ValueError(f"nlosgr: IRF center {center} outside [0, {L})")
        self.taps = t.to(torch.float32).contiguous()
        self.center = center
        self.background = float(background)

    def __len__(self):
        return self.taps.numel()

    @property
    def device(self):
        return self.taps.device

    def to(self, device):
        if torch.device(device) == self.taps.device:
            return self
        return IRF(self.taps.to(device), self.center, self.background)

    def normalized(self):
        """The same response with taps of sum 1."""
        s = self.taps.double().sum()
        return IRF((self.taps.double() / s).float(), self.center, self.background)

    def struct(self):
        """The nlosgr_irf of device taps (keep self alive until the call is enqueued)."""
        return _lib.Irf(len(self), self.center, _lib.ptr(self.taps), self.background)

    def __repr__(self):
        return f"IRF(taps={len(self)}, center={self.center}, background={self.background})"


def gaussian_irf(fwhm_bins, tail_bins=0.0, truncate=4.0, background=0.0):
    """A Gaussian of the given FWHM (bins), convolved with the one-sided exponential exp(-k / tail_bins),
    k >= 0, when tail_bins > 0; each truncated at `truncate` widths (sigma / decay), normalised to sum 1
    and centred at its peak."""
    if not fwhm_bins > 0:
        raise ValueError("nlosgr: fwhm_bins must be > 0")
    sigma = float(fwhm_bins) / (2.0 * math.sqrt(2.0 * math.log(2.0)))
    n = max(1, int(math.ceil(truncate * sigma)))
    k = np.arange(-n, n + 1, dtype=np.float64)
    w = np.exp(-0.5 * (k / sigma) ** 2)
    if tail_bins > 0:
        nt = max(1, int(math.ceil(truncate * tail_bins)))
        w = np.convolve(w, np.exp(-np.arange(nt + 1, dtype=np.float64) / float(tail_bins)))
    if w.size > MAX_TAPS:
        raise ValueError(f"nlosgr: this response needs {w.size} taps (> {MAX_TAPS}); lower truncate")
    w = w / w.sum()
    return IRF(w, int(np.argmax(w)), background)


def _conv_cpu(x, irf, adjoint):
    """The two sums through torch.nn.functional.conv1d (a correlation: weight k meets input t + k - pad_left)."""
    L, c = len(irf), irf.center
    w = irf.taps.to(device=x.device, dtype=x.dtype)
    if adjoint:
        pl, pr, k = c, L - 1 - c, w
    else:
        pl, pr, k = L - 1 - c, c, w.flip(0)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x.unsqueeze(1), (pl, pr)), k.view(1, 1, L)).squeeze(1)
    return y if adjoint else y + irf.background


def irf_apply(x, irf, adjoint=False):
    """apply (or adjoint) of a float32 GPU tensor [rows, nr] through nlosgr_irf_apply; no autograd."""
    lib = _lib.load()
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("nlosgr: irf_apply takes a float32 GPU tensor [rows, nr]")
    x = x.detach().contiguous()
    irf = irf.to(x.device)
    y = torch.empty_like(x)
    s = irf.struct()
    _lib.check(lib.nlosgr_irf_apply(_lib.ptr(x), x.shape[0], x.shape[1], ctypes.byref(s), int(bool(adjoint)),
                                    _lib.ptr(y), _lib.stream_handle(x.device)))
    return y


class _ConvolveTime(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, irf):
        ctx.irf = irf
        return irf_apply(x, irf, False)

    @staticmethod
    def backward(ctx, g):
        return irf_apply(g.float(), ctx.irf, True), None


def convolve_time(hist, irf):
    """y = apply(hist) along the last axis, differentiable in hist.  GPU float32 tensors go through
    nlosgr_irf_apply (backward: the same call with adjoint = 1); CPU tensors (any float dtype) fall back
    to conv1d with the same convention.  This is also how a render becomes a synthetic capture."""
    shape = hist.shape
    x = hist.reshape(1, -1) if hist.dim() < 2 else hist.reshape(-1, shape[-1])
    if x.is_cuda:
        if x.dtype != torch.float32:
            raise ValueError("nlosgr: convolve_time on the GPU takes float32")
        y = _ConvolveTime.apply(x, irf.to(x.device))
    else:
        y = _conv_cpu(x, irf, False)
    return y.reshape(shape)


def adjoint_time(z, irf):
    """g = adjoint(z) along the last axis (no background): the transpose of convolve_time's linear part."""
    shape = z.shape
    x = z.reshape(1, -1) if z.dim() < 2 else z.reshape(-1, shape[-1])
    y = irf_apply(x, irf, True) if x.is_cuda else _conv_cpu(x, irf, True)
    return y.reshape(shape)
