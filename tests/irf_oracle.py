"""Float64 restatement of the temporal instrument response (include/nlosgr.h, ABI 12), as plain numpy
loops over the taps, built from the same fp32 inputs the kernels read:

    apply:    y[p,t] = b + sum_j w[j] h[p, t + c - j]      (h = 0 outside [0, nr))
    adjoint:  g[p,s] =     sum_j w[j] z[p, s - c + j]      (z = 0 outside [0, nr))

and the running-error bounds of the fp32 kernels that the GPU tests hold them to.  An L-term fp32 sum
of products, formed in any order with or without fma, is within (L + 2) u of the exact sum times the sum
of the terms' magnitudes, u = 2^-24 (one rounding per product, at most L - 1 per add chain, one for the
background; second-order terms are far below the slack of the + 2).
"""
import numpy as np

U = 2.0 ** -24


def _shifted_acc(out, src, wj, shift, tmp=None):
    """out[:, t] += wj * src[:, t + shift] where 0 <= t + shift < nr."""
    nr = src.shape[1]
    lo, hi = max(0, -shift), min(nr, nr - shift)
    if hi > lo:
        if tmp is None:
            out[:, lo:hi] += wj * src[:, lo + shift:hi + shift]
        else:
            t = tmp[:, :hi - lo]
            np.multiply(src[:, lo + shift:hi + shift], wj, out=t)
            out[:, lo:hi] += t


def _tap_loop(src, w, shifts):
    """sum_j w[j] src[:, t + shifts[j]], the loop over the taps run per block of rows (cache-sized: the
    arithmetic is the same, a 257 x 8192 volume just does not stream through memory once per tap)."""
    src = np.ascontiguousarray(src, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    out = np.zeros_like(src)
    rows, nr = src.shape
    step = max(1, 32768 // max(1, nr))
    tmp = np.empty((step, nr))
    for r0 in range(0, rows, step):
        s, o = src[r0:r0 + step], out[r0:r0 + step]
        for j in range(w.size):
            _shifted_acc(o, s, w[j], shifts[j], tmp[:s.shape[0]])
    return out


def apply64(h, w, c, b=0.0):
    return _tap_loop(h, w, [c - j for j in range(len(w))]) + float(b)


def adjoint64(z, w, c):
    return _tap_loop(z, w, [j - c for j in range(len(w))])


def apply_bound(h, w, c, b=0.0):
    """(bound, A): |y_fp32 - y64| <= (L + 2) 2^-24 A per element, A = |b| + (|w| * |h|)."""
    A = apply64(np.abs(np.asarray(h, dtype=np.float64)), np.abs(np.asarray(w, dtype=np.float64)), c, abs(float(b)))
    return (len(w) + 2) * U * A, A


def adjoint_bound(z, w, c):
    A = adjoint64(np.abs(np.asarray(z, dtype=np.float64)), np.abs(np.asarray(w, dtype=np.float64)), c)
    return (len(w) + 2) * U * A, A


def loss_irf64(hist, target, gt_times, w, c, b):
    """(loss, equal_loss) of the fused loss in float64."""
    t = np.asarray(target, dtype=np.float64) * float(gt_times)
    d = apply64(hist, w, c, b) - t
    loss = float((d * d).mean())
    return np.array([loss, loss / float((t * t).mean())])


def mse_irf64(hist, target, gt_times, w, c, b, grad_scale, y=None, A=None):
    """(loss4 [4] float64, grad [rows, nr] float64, bound on the fp32 gradient's error per element):
    d = y - gt target, grad = adjoint(grad_scale 2 d / n); the bound is (2L + 8) 2^-24 S with
    S = gscale adjoint_|w|(A + |gt target|): the apply's (L + 2) u A reaches d, the subtraction, the target's
    product and the scale (with gscale's own rounding) add 4 u (A + |gt t|), and the adjoint's own (L + 2) u acts
    on |z| <= gscale (A + |gt t|).  y, A: apply64 / apply_bound of the same inputs when the caller has them."""
    hist = np.asarray(hist, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64) * float(gt_times)
    n = hist.size
    y = apply64(hist, w, c, b) if y is None else y
    d = y - t
    se, st = float((d * d).sum()), float((t * t).sum())
    loss = se / n
    loss4 = np.array([loss, loss / (st / n) if st > 0 else 0.0, se, st])
    gscale = float(grad_scale) * 2.0 / n
    grad = adjoint64(gscale * d, w, c)
    if A is None:
        _, A = apply_bound(hist, w, c, b)
    S = gscale * adjoint64(A + np.abs(t), np.abs(np.asarray(w, dtype=np.float64)), c)
    return loss4, grad, (2 * len(w) + 8) * U * S


def emulate_apply32(h, w, c, b=0.0):
    """The kernel's arithmetic in fp32 on the CPU: a sequential fma chain over ascending taps started at 0
    (each fma formed exactly in float64 and rounded once: the product of two fp32 is exact in float64, and
    the double rounding of the sum is harmless at this level), then + b."""
    h = np.asarray(h, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    acc = np.zeros(h.shape, dtype=np.float32)
    for j in range(w.size):
        term = np.zeros(h.shape, dtype=np.float64)
        _shifted_acc(term, h.astype(np.float64), float(w[j]), c - j)
        acc = (acc.astype(np.float64) + term).astype(np.float32)
    return (acc + np.float32(b)).astype(np.float32)
