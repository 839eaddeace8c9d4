"""A primal-dual solver (Chambolle-Pock, theta = 1) for

    minimise over v (>= 0 by default)   F(A v) + tv sum_voxels |a o grad v|_2 + l1 sum |v|

on a volume [W, nr, H] with rows [H W, nr], over two callables A and A^T.  F is the MSE 1/2 |z - h|^2 or the Poisson
term of a photon-count histogram with a per-bin exposure e (the falloff of a confocal capture belongs there, not on
the counts):  y' = max(gt_times h, 0) + eps, rho = e z + eps, F = sum [rho - y' + y' log(y'/rho)], the y', rho and
eps = rate_floor of the training loss (nlosgr.loss, loss="poisson").  The gradient is forward differences in index
units with a weight per axis (n, j, m) and 0 at an axis's last index; include/nlosgr.h, "Primal-dual passes", states
every formula.  One iteration, with x the iterate, xbar the extrapolated point, q the row dual and p [3, W, nr, H]
the TV dual:

    z = A xbar;  q <- prox_{sigma F*}(q + sigma z)                       prox_rows        nlosgr_prox_rows
                 p <- project_{|p|_2 <= tv}(p + sigma a o grad xbar)     tv_dual_step     nlosgr_tv_dual
    g = A^T q;   x+ = shrink(x - tau (g + (a o grad)^T p), tau l1), clamped at 0 with nonneg
                 xbar <- 2 x+ - x;  x <- x+                              tv_primal_step   nlosgr_tv_primal

Everything that is not an operator application is one of three HIP passes (csrc/nlosgr_prox.hip), each one launch, in
place, without atomics: bitwise repeatable.  The two dual passes emit the objective's terms at the point the operator
was applied to, in double.  No CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from .lattice import _extents, _gpu

INF = float("inf")


def _weights(weights):
    w = tuple(float(np.float32(v)) for v in weights)
    if len(w) != 3 or not all(np.isfinite(v) and v >= 0 for v in w):
        raise ValueError("nlosgr: weights must be three finite values >= 0, for the axes (n, j, m)")
    return w


def _volume(t, what, shape=None, device=None):
    if isinstance(t, torch.Tensor) and not t.is_contiguous():
        raise ValueError(f"nlosgr: {what} is updated in place: it takes contiguous tensors")
    t = _gpu(t, torch.float32, what)
    if (shape is None and t.dim() != 3) or (shape is not None and (tuple(t.shape) != tuple(shape) or t.device != device)):
        raise ValueError(f"nlosgr: {what} takes float32 volumes [W, nr, H]" if shape is None else
                         f"nlosgr: {what}: a tensor must be float32 {tuple(shape)} on {device}")
    return t


def _loss(loss):
    if loss not in _lib.LOSSES:
        raise ValueError(f"nlosgr: loss must be one of {tuple(_lib.LOSSES)}")
    return _lib.LOSSES[loss]


def _exposure(exposure, kind, nr, device):
    if exposure is None:
        return None
    if kind == _lib.LOSS_MSE:
        raise ValueError("nlosgr: the MSE data term takes no exposure")
    e = _gpu(exposure, torch.float32, "prox_rows (exposure)")
    if tuple(e.shape) != (nr,) or e.device != device:
        raise ValueError(f"nlosgr: exposure must be float32 [{nr}] on {device}")
    return e


@torch.no_grad()
def prox_rows(q, z, h, H, W, sigma, loss="mse", exposure=None, gt_times=1.0, rate_floor=1.0):
    """q <- prox_{sigma F*}(q + sigma z), in place, for rows [H W, nr] (nlosgr_prox_rows).  h: the target rows;
    exposure: fp32 [nr], finite and >= 0 (Poisson only; None: ones).  Returns F(z), a float64 scalar on the device
    (Poisson: with rho = max(e z, 0) + eps)."""
    lib = _lib.load()
    kind = _loss(loss)
    if isinstance(q, torch.Tensor) and not q.is_contiguous():
        raise ValueError("nlosgr: prox_rows updates q in place: it takes a contiguous tensor")
    q, z, h = (_gpu(t, torch.float32, "prox_rows") for t in (q, z, h))
    if q.dim() != 2:
        raise ValueError("nlosgr: prox_rows takes rows [H W, nr]")
    H, W, nr = _extents(H, W, q.shape[1])
    if not (tuple(q.shape) == tuple(z.shape) == tuple(h.shape) == (H * W, nr)) or not (q.device == z.device == h.device):
        raise ValueError(f"nlosgr: q, z and h must be float32 [{H * W}, {nr}] on one device")
    e = _exposure(exposure, kind, nr, q.device)
    part = torch.empty(int(lib.nlosgr_prox_rows_partials(H, W, nr)), dtype=torch.float64, device=q.device)
    _lib.check(lib.nlosgr_prox_rows(_lib.ptr(z), _lib.ptr(h), _lib.ptr(e), H, W, nr, kind, float(gt_times),
                                    float(rate_floor), float(sigma), _lib.ptr(q), _lib.ptr(part),
                                    _lib.stream_handle(q.device)))
    return part.sum()


@torch.no_grad()
def tv_dual_step(p, xbar, sigma, tv, weights=(1.0, 1.0, 1.0)):
    """p <- project_{|p|_2 <= tv}(p + sigma a o grad xbar), in place, p [3, W, nr, H] (nlosgr_tv_dual).  tv = 0
    writes zeros, tv = inf never projects.  Returns float64 [2] on the device: sum |a o grad xbar|_2, sum |xbar|."""
    lib = _lib.load()
    xbar = _volume(xbar, "tv_dual_step")
    W, nr, H = (int(v) for v in xbar.shape)
    _extents(H, W, nr)
    p = _volume(p, "tv_dual_step", (3, W, nr, H), xbar.device)
    a = _weights(weights)
    part = torch.empty((int(lib.nlosgr_tv_dual_partials(W, nr, H)) // 2, 2), dtype=torch.float64, device=xbar.device)
    _lib.check(lib.nlosgr_tv_dual(_lib.ptr(xbar), W, nr, H, a[0], a[1], a[2], float(sigma), float(tv), _lib.ptr(p),
                                  _lib.ptr(part), _lib.stream_handle(xbar.device)))
    return part.sum(dim=0)


@torch.no_grad()
def tv_primal_step(x, xbar, g, p, tau, l1=0.0, weights=(1.0, 1.0, 1.0), nonneg=True):
    """x+ = shrink(x - tau (g + (a o grad)^T p), tau l1), clamped at 0 with nonneg; xbar <- 2 x+ - x; x <- x+; both
    in place (nlosgr_tv_primal).  Returns (x, xbar)."""
    lib = _lib.load()
    x = _volume(x, "tv_primal_step")
    W, nr, H = (int(v) for v in x.shape)
    _extents(H, W, nr)
    xbar = _volume(xbar, "tv_primal_step", (W, nr, H), x.device)
    g = _volume(g, "tv_primal_step", (W, nr, H), x.device)
    p = _volume(p, "tv_primal_step", (3, W, nr, H), x.device)
    a = _weights(weights)
    _lib.check(lib.nlosgr_tv_primal(_lib.ptr(g), _lib.ptr(p), W, nr, H, a[0], a[1], a[2], float(tau), float(l1),
                                    1 if nonneg else 0, _lib.ptr(x), _lib.ptr(xbar), _lib.stream_handle(x.device)))
    return x, xbar


@torch.no_grad()
def tv_gradient(x, weights=(1.0, 1.0, 1.0)):
    """a o grad x, fp32 [3, W, nr, H]: the dual pass with p = 0, sigma = 1 and tv = inf."""
    x = _volume(x, "tv_gradient")
    p = torch.zeros((3,) + tuple(x.shape), device=x.device)
    tv_dual_step(p, x, 1.0, INF, weights)
    return p


@torch.no_grad()
def tv_divergence(p, weights=(1.0, 1.0, 1.0)):
    """(a o grad)^T p, fp32 [W, nr, H], the exact transpose of tv_gradient: the primal pass with x = g = 0, tau = 1,
    l1 = 0 and no clamp, negated."""
    p = _gpu(p, torch.float32, "tv_divergence")
    if p.dim() != 4 or p.shape[0] != 3:
        raise ValueError("nlosgr: tv_divergence takes p [3, W, nr, H]")
    x = torch.zeros(tuple(p.shape[1:]), device=p.device)
    tv_primal_step(x, torch.empty_like(x), torch.zeros_like(x), p, 1.0, 0.0, weights, nonneg=False)
    return x.neg_()


def default_steps(norm_A, tv=0.0, weights=(1.0, 1.0, 1.0)):
    """tau = sigma = 1 / sqrt(L), L = norm_A + 4 sum a^2 (the second part with tv > 0 only): an upper bound of the
    squared norm of the stacked operator (A; a o grad), given that norm_A bounds |A|^2 from above."""
    L = float(norm_A) + (4.0 * sum(v * v for v in _weights(weights)) if float(tv) > 0 else 0.0)
    if not (L > 0 and np.isfinite(L)):
        raise ValueError("nlosgr: norm_A must be finite and > 0")
    return 1.0 / np.sqrt(L)


@torch.no_grad()
def primal_dual(h, forward, adjoint, volume_shape, norm_A, iterations, tv=0.0, l1=0.0, loss="mse", exposure=None,
                gt_times=1.0, rate_floor=1.0, weights=(1.0, 1.0, 1.0), nonneg=True, tau=None, sigma=None, x0=None):
    """(volume [W, nr, H], objective [iterations] float64, terms [iterations, 3] float64), the last two on the device:
    `iterations` Chambolle-Pock steps (the module's docstring) from x0 (zeros by default) with q = 0 and p = 0.
    forward(volume) -> rows [H W, nr] and adjoint(rows) -> volume are A and A^T (fp32 GPU tensors; neither may keep
    or change its argument); norm_A: an upper bound of |A|^2.  tau, sigma: the steps, default_steps' by default
    (tau sigma L <= 1 is the condition of convergence).  terms[n] = (F(A xbar_n), sum |a o grad xbar_n|_2,
    sum |xbar_n|) at the point xbar_n the operator is applied to, BEFORE update n (lct_solve's convention), and
    objective[n] = terms[n] . (1, tv, l1).  No host read inside the loop."""
    kind = _loss(loss)
    h = _gpu(h, torch.float32, "primal_dual")
    W, nr, H = (int(v) for v in volume_shape)
    _extents(H, W, nr)
    if tuple(h.shape) != (H * W, nr):
        raise ValueError(f"nlosgr: the rows must be float32 [{H * W}, {nr}] for a volume {(W, nr, H)}")
    if not (0 <= float(tv) < INF and 0 <= float(l1) < INF):
        raise ValueError("nlosgr: tv and l1 must be finite and >= 0")
    if int(iterations) < 1:
        raise ValueError("nlosgr: iterations must be >= 1")
    a = _weights(weights)
    e = _exposure(exposure, kind, nr, h.device)
    step = default_steps(norm_A, tv, a)
    tau = step if tau is None else float(tau)
    sigma = step if sigma is None else float(sigma)
    if x0 is None:
        x = torch.zeros((W, nr, H), device=h.device)
    else:
        x = _gpu(x0, torch.float32, "primal_dual").clone()
        if tuple(x.shape) != (W, nr, H):
            raise ValueError(f"nlosgr: x0 must have the volume's shape {(W, nr, H)}")
    xbar = x.clone()
    q = torch.zeros_like(h)
    p = torch.zeros((3, W, nr, H), device=h.device)
    terms = torch.zeros((int(iterations), 3), dtype=torch.float64, device=h.device)
    for n in range(int(iterations)):
        z = forward(xbar)
        terms[n, 0] = prox_rows(q, z, h, H, W, sigma, loss, e, gt_times, rate_floor)
        terms[n, 1:] = tv_dual_step(p, xbar, sigma, tv, a)
        del z
        tv_primal_step(x, xbar, adjoint(q), p, tau, l1, a, nonneg)
    objective = terms[:, 0] + float(tv) * terms[:, 1] + float(l1) * terms[:, 2]
    return x, objective, terms
