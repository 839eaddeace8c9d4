"""Float64 numpy restatement of the primal-dual passes (include/nlosgr.h, "Primal-dual passes"; nlosgr.prox) and of
the Chambolle-Pock loop over lct_op_oracle.Operator64, fed the same fp32 inputs the kernels get.

    volume [W, nr, H], axes (n, j, m);  a = (a_n, a_j, a_m)
    grad(x, a)[k]   = a_k (x[i + e_k] - x[i]) where i_k < N_k - 1, else 0             [3, W, nr, H]
    grad_t(p, a)    = sum_k a_k ((i_k > 0 ? p_k[i - e_k] : 0) - (i_k < N_k - 1 ? p_k[i] : 0))
    project(u, tv)  = u where |u|_2 <= tv, else u tv / |u|_2; zeros for tv = 0
    prox_mse        = (u - sigma h) / (1 + sigma)
    prox_poisson    = d 2 (s - s' y') / (1 + s + D),  s' = sigma / d^2, s = u / d + s' eps,
                      D = sqrt((s - 1)^2 + 4 s' y'), y' = max(gt h, 0) + eps;  0 where d = 0;
                      1 + s + D as 2 + 4 s' y' / (D + 1 - s) where s <= 1 (no cancellation)
"""
import numpy as np


def grad(x, a=(1.0, 1.0, 1.0)):
    x = np.asarray(x, dtype=np.float64)
    g = np.zeros((3,) + x.shape)
    g[0, :-1] = a[0] * (x[1:] - x[:-1])
    g[1, :, :-1] = a[1] * (x[:, 1:] - x[:, :-1])
    g[2, :, :, :-1] = a[2] * (x[:, :, 1:] - x[:, :, :-1])
    return g


def grad_t(p, a=(1.0, 1.0, 1.0)):
    """The exact transpose of grad; p_k at the last index of axis k is never read."""
    p = np.asarray(p, dtype=np.float64)
    out = np.zeros(p.shape[1:])
    for k in range(3):
        q = np.moveaxis(p[k], k, 0)
        t = np.zeros(q.shape)
        t[1:] += q[:-1]
        t[:-1] -= q[:-1]
        out += a[k] * np.moveaxis(t, 0, k)
    return out


def grad_t_abs(p, a=(1.0, 1.0, 1.0)):
    """The sum of the absolute terms of grad_t (the scale of its rounding error)."""
    p = np.abs(np.asarray(p, dtype=np.float64))
    out = np.zeros(p.shape[1:])
    for k in range(3):
        q = np.moveaxis(p[k], k, 0)
        t = np.zeros(q.shape)
        t[1:] += q[:-1]
        t[:-1] += q[:-1]
        out += a[k] * np.moveaxis(t, 0, k)
    return out


def norm3(u):
    return np.sqrt((np.asarray(u, dtype=np.float64) ** 2).sum(axis=0))


def project(u, tv):
    u = np.asarray(u, dtype=np.float64)
    if tv == 0:
        return np.zeros(u.shape)
    n = norm3(u)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(n <= tv, 1.0, tv / np.where(n > 0, n, 1.0))
    return u * f[None]


def tv_sum(x, a=(1.0, 1.0, 1.0)):
    return float(norm3(grad(x, a)).sum())


def shrink(u, thr, nonneg):
    if nonneg:
        return np.maximum(u - thr, 0.0)
    return np.sign(u) * np.maximum(np.abs(u) - thr, 0.0)


def exposure64(e, nr):
    return np.ones(nr) if e is None else np.asarray(e, dtype=np.float64)


def counts64(h, gt, eps):
    return np.maximum(float(gt) * np.asarray(h, dtype=np.float64), 0.0) + float(eps)


def prox_mse(u, h, sigma):
    return (np.asarray(u, dtype=np.float64) - sigma * np.asarray(h, dtype=np.float64)) / (1.0 + sigma)


def prox_poisson(u, h, sigma, e=None, gt=1.0, eps=1.0):
    """prox of sigma F* at u [rows, nr], the cancellation-free closed form."""
    u = np.asarray(u, dtype=np.float64)
    d = np.broadcast_to(exposure64(e, u.shape[-1]), u.shape)
    yp = counts64(h, gt, eps)
    ds = np.where(d > 0, d, 1.0)
    sp = sigma / ds ** 2
    s = u / ds + sp * eps
    A, c = s - 1.0, 4.0 * sp * yp
    D = np.sqrt(A * A + c)
    den = np.where(A > 0, 2.0 + A + D, 2.0 + c / (D - np.minimum(A, 0.0)))       # 1 + s + D without cancellation
    return np.where(d > 0, ds * 2.0 * (s - sp * yp) / den, 0.0)


def prox_poisson_residual(q, u, h, sigma, e=None, gt=1.0, eps=1.0):
    """The optimality condition of the prox.  By Moreau's identity q = u - sigma z with z the minimiser of
    F(z) + sigma / 2 (z - u / sigma)^2, so F'(z) = q at z = (u - q) / sigma, and F'(z) = d (1 - y' / rho) with
    rho = d z + eps.  In q' = q / d, s' = sigma / d^2, s = u / d + s' eps that is (1 - q') (s - q') = s' y' with
    q' < 1.  Returns the residual of that equation relative to the sum of its absolute terms,
    (1 + |q'|) (|s| + |q'|) + s' y', where d > 0, and |q| where d = 0."""
    u = np.asarray(u, dtype=np.float64)
    d = np.broadcast_to(exposure64(e, u.shape[-1]), u.shape)
    yp = counts64(h, gt, eps)
    ds = np.where(d > 0, d, 1.0)
    sp = sigma / ds ** 2
    s, qp = u / ds + sp * eps, q / ds
    res = np.abs((1.0 - qp) * (s - qp) - sp * yp) / ((1.0 + np.abs(qp)) * (np.abs(s) + np.abs(qp)) + sp * yp)
    return np.where(d > 0, res, np.abs(q))


def data_term(z, h, loss="mse", e=None, gt=1.0, eps=1.0):
    """F(z) as the rows pass reports it (Poisson: rho = max(e z, 0) + eps)."""
    z, h = np.asarray(z, dtype=np.float64), np.asarray(h, dtype=np.float64)
    if loss == "mse":
        return 0.5 * float(((z - h) ** 2).sum())
    yp = counts64(h, gt, eps)
    rho = np.maximum(exposure64(e, z.shape[-1])[None] * z, 0.0) + eps
    t = (rho - yp) / yp
    return float((yp * (t - np.log1p(t))).sum())


def functional(op, x, h, tv=0.0, l1=0.0, loss="mse", e=None, gt=1.0, eps=1.0, a=(1.0, 1.0, 1.0)):
    """(Phi, F, TV, L1) of a volume x under operator op (forward only)."""
    x = np.asarray(x, dtype=np.float64)
    F = data_term(op.forward(x), h, loss, e, gt, eps)
    T, L = tv_sum(x, a), float(np.abs(x).sum())
    return F + tv * T + l1 * L, F, T, L


def default_step(norm_A, tv, a=(1.0, 1.0, 1.0)):
    return 1.0 / np.sqrt(norm_A + (4.0 * sum(v * v for v in a) if tv > 0 else 0.0))


def primal_dual(op, h, iterations, norm_A, tv=0.0, l1=0.0, loss="mse", e=None, gt=1.0, eps=1.0, a=(1.0, 1.0, 1.0),
                nonneg=True, tau=None, sigma=None):
    """(volume, objective [iterations], terms [iterations, 3]) of nlosgr.prox.primal_dual over op.forward and
    op.adjoint, from zeros."""
    h = np.asarray(h, dtype=np.float64)
    step = default_step(norm_A, tv, a)
    tau = step if tau is None else tau
    sigma = step if sigma is None else sigma
    x = np.zeros((op.W, op.nr, op.H))
    xbar, q, p = x.copy(), np.zeros(h.shape), np.zeros((3,) + x.shape)
    terms = np.zeros((iterations, 3))
    for n in range(iterations):
        z = op.forward(xbar)
        terms[n] = (data_term(z, h, loss, e, gt, eps), tv_sum(xbar, a), np.abs(xbar).sum())
        u = q + sigma * z
        q = prox_mse(u, h, sigma) if loss == "mse" else prox_poisson(u, h, sigma, e, gt, eps)
        p = project(p + sigma * grad(xbar, a), tv)
        xn = shrink(x - tau * (op.adjoint(q) + grad_t(p, a)), tau * l1, nonneg)
        xbar, x = 2.0 * xn - x, xn
    return x, terms @ np.array([1.0, tv, l1]), terms


def lambda0(op, h, loss="mse", e=None, gt=1.0, eps=1.0):
    """max(-A^T grad F(0)): above it (as l1, with nonneg) the zero volume is the minimiser."""
    h = np.asarray(h, dtype=np.float64)
    if loss == "mse":
        return float(op.adjoint(h).max())
    yp = counts64(h, gt, eps)
    return float(op.adjoint(exposure64(e, h.shape[-1])[None] * (yp / eps - 1.0)).max())


def converged_norm(op, tol=1e-10, most=5000):
    """The largest eigenvalue of A^T A: Operator64's power iteration run until the estimate moves by less than
    tol (relative) between iterations."""
    v = np.ones((op.W, op.nr, op.H))
    lam = 0.0
    for _ in range(most):
        v = v / np.sqrt((v * v).sum())
        v = op.adjoint(op.forward(v))
        new = float(np.sqrt((v * v).sum()))
        if abs(new - lam) <= tol * new:
            return new
        lam = new
    return lam
