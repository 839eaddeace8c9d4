"""Float64 restatement of the photon-count likelihood of the fused loss (include/nlosgr.h, nlosgr_loss_irf with
NLOSGR_LOSS_POISSON), built from the same fp32 inputs the kernel reads, on top of tests/irf_oracle.py:

    lambda = b + sum_j w[j] h[p, t + c - j]                 (irf_oracle.apply64)
    y'  = max(gt t, 0) + eps        rho = max(lambda, 0) + eps
    dev = 2 [y' log(y'/rho) - (y' - rho)]  =  2 y' (e - log1p(e)),   e = (rho - y') / y'
    z   = gscale (rho - y') / rho  where lambda >= 0, else 0,       gscale = grad_scale 2 / n
    grad = adjoint(z)                                       (irf_oracle.adjoint64)
    loss4 = {sum dev / n, sum dev / sum max(gt t, 0) (0 without counts), sum dev, sum max(gt t, 0)}

and the bound the GPU test holds the fp32 gradient to, u = 2^-24.  The kernel's element sequence is prescribed,
one fp32 rounding per operation:

    y = gt t;  y' = max(y, 0) + eps;  rho = max(lambda, 0) + eps;  r = rho - y';  z = gscale (r / rho)

  * lambda carries the apply's error E = (L + 2) u A (irf_oracle.apply_bound); max(., 0) does not enlarge it, and
    the add of eps rounds once: |rho^ - rho| <= E + u rho.
  * y' carries two roundings (the product, the add): |y'^ - y'| <= 2 u y'.
  * q = (rho - y') / rho = 1 - y'/rho has dq/drho = y'/rho^2 and dq/dy' = -1/rho, and the subtraction and the
    division (correctly rounded: the library is built without fast math, and HIP's fp32 division is correctly
    rounded by default) add u |q| each:
        |q^ - q| <= (y'/rho) E / rho + u y'/rho + 2 u y'/rho + 2 u |q|
    With y'/rho = 1 - q <= 1 + |q| this is at most (1 + |q|) E / rho + u (1 + 2 y'/rho) + 3 u |q|.
  * gscale is formed in double and rounded to fp32, and the product with q^ rounds once: 2 u |q| more.
  * One further u |q| stands for the second-order terms, which makes the 6:
        dz = gscale [ (1 + |q|) E / rho + u (1 + 2 y'/rho) + 6 u |q| ]
  * The adjoint is linear: it carries dz through |w|, and adds its own running error (L + 2) u on |z|:
        bound = adjoint_|w|(dz) + (L + 2) u adjoint_|w|(|z|)

The bound is first order in E / rho, and it assumes the fp32 lambda and the float64 one fall on the same side of
0; callers whose taps can make lambda negative keep |lambda| well above E (the GPU test asserts 10 E).
"""
import numpy as np

import irf_oracle as IO

U = IO.U


def elements64(lam, target, gt_times, eps):
    """(y', rho, dev, q, ycount) per element in float64; q = (rho - y') / rho where lambda >= 0 else 0."""
    lam = np.asarray(lam, dtype=np.float64)
    y = np.asarray(target, dtype=np.float64) * float(np.float32(gt_times))
    eps = float(np.float32(eps))
    ycount = np.maximum(y, 0.0)
    yp = ycount + eps
    rho = np.maximum(lam, 0.0) + eps
    e = (rho - yp) / yp
    dev = 2.0 * yp * (e - np.log1p(e))
    q = np.where(lam >= 0.0, (rho - yp) / rho, 0.0)
    return yp, rho, dev, q, ycount


def deviance64(rho, yp):
    """The textbook form 2 [y' log(y'/rho) - (y' - rho)] (the identities test compares the two)."""
    rho = np.asarray(rho, dtype=np.float64)
    yp = np.asarray(yp, dtype=np.float64)
    return 2.0 * (yp * np.log(yp / rho) - (yp - rho))


def poisson_irf64(hist, target, gt_times, w, c, b, eps, grad_scale, y=None, A=None):
    """(loss4 [4] float64, grad [rows, nr] float64, bound on the fp32 gradient's error per element, lambda64).
    y, A: apply64 / apply_bound's A of the same inputs when the caller has them."""
    hist = np.asarray(hist, dtype=np.float64)
    n = hist.size
    L = len(w)
    lam = IO.apply64(hist, w, c, b) if y is None else y
    if A is None:
        _, A = IO.apply_bound(hist, w, c, b)
    yp, rho, dev, q, ycount = elements64(lam, target, gt_times, eps)
    sd, sy = float(dev.sum()), float(ycount.sum())
    loss4 = np.array([sd / n if n else 0.0, sd / sy if sy > 0 else 0.0, sd, sy])
    gscale = float(grad_scale) * 2.0 / n if n else 0.0
    z = gscale * q
    grad = IO.adjoint64(z, w, c)
    E = (L + 2) * U * A
    aq = np.abs(q)
    dz = gscale * ((1.0 + aq) * E / rho + U * (1.0 + 2.0 * yp / rho) + 6.0 * U * aq)
    dz = np.where(lam >= 0.0, dz, 0.0)               # a clamped element is exactly 0 on both sides
    aw = np.abs(np.asarray(w, dtype=np.float64))
    bound = IO.adjoint64(dz + (L + 2) * U * np.abs(z), aw, c)        # both terms in one pass: the adjoint is linear
    return loss4, grad, bound, lam


def loss64(hist, target, gt_times, w, c, b, eps, grad_scale=1.0):
    """grad_scale * mean deviance, a scalar function of hist (the central-difference test differentiates it)."""
    lam = IO.apply64(hist, w, c, b)
    _, _, dev, _, _ = elements64(lam, target, gt_times, eps)
    return float(grad_scale) * float(dev.sum()) / dev.size


def emulate_poisson32(lam32, target, gt_times, eps, gscale):
    """The kernel's element sequence in numpy fp32 (one rounding per operation) from an fp32 lambda:
    (z fp32, dev fp32).  log1p is numpy's fp32 one, not the device's."""
    f = np.float32
    lam = np.asarray(lam32, dtype=f)
    y = f(gt_times) * np.asarray(target, dtype=f)
    yp = np.maximum(y, f(0)) + f(eps)
    rho = np.maximum(lam, f(0)) + f(eps)
    r = rho - yp
    z = np.where(lam >= 0, f(gscale) * (r / rho), f(0)).astype(f)
    e = np.maximum(r / yp, f(-1) + f(2.0 ** -24))
    dev = (f(2) * yp * (e - np.log1p(e))).astype(f)
    return z, dev
