"""Float64 numpy restatement of the LCT operator pair (include/nlosgr.h, "LCT operator pair"; the symbols
nlosgr_lct_load_volume / _store_rows / _load_rows / _store_volume and nlosgr.lct.LctOperator), fed the same fp32 inputs
the kernels get.  It is built from the parts of tests/lct_oracle.py (resampling64, kernel64) and the lattices of
tests/fk_oracle.py.

    w_j  = (r0 + j dr)^power, power in -4..4; a negative power gives 0 where r <= 0
    A    : volume [W, nr, H] -> rows [H W, nr]
           g[m, n, i]       = sum_j R[i, j] volume[n, j, m]
           o                = Re ifftn( fftn(pad g) Fk ),   Fk = fftn(K)
           rows[v(m, n), j] = w_j sum_i R[i, j] o[m, n, i]
    A^T  : rows -> volume
           g[m, n, i]       = sum_j R[i, j] (w_j rows[v, j])
           o                = Re ifftn( fftn(pad g) conj(Fk) )
           volume[n, j, m]  = sum_i R[i, j] o[m, n, i]

Nothing is clamped.  R may be passed in (the operator's own fp32 weights as float64, Resampling.dense()), so that
the weights' rounding is not charged to a kernel."""
import functools

import numpy as np

import fk_oracle as FO
import lct_oracle as LO


def weights64(r0, dr, nr, power):
    """w [nr] float64 from the fp32 r0 and dr."""
    r = FO.f32(r0) + np.arange(nr) * FO.f32(dr)
    power = int(power)
    if power >= 0:
        return r ** power
    with np.errstate(divide="ignore"):
        return np.where(r > 0, 1.0 / np.where(r > 0, r, 1.0) ** (-power), 0.0)


class Operator64:
    """A and A^T of one lattice and window in float64; R: [nv, nr] float64 (None: lct_oracle.resampling64's)."""

    def __init__(self, H, W, sx, sz, r0, dr, nr, power=0, nv=None, perm=None, x_along="n", R=None):
        self.H, self.W, self.nr = H, W, nr
        R64, self.dv = LO.resampling64(r0, dr, nr, nv)
        self.R = R64 if R is None else np.asarray(R, dtype=np.float64)
        assert self.R.shape == R64.shape
        self.nv = self.R.shape[0]
        K, self.scale = LO.kernel64(H, W, self.nv, sx, sz, self.dv)
        self.Fk = np.fft.fftn(K)
        self.w = weights64(r0, dr, nr, power)
        self.v = FO.lattice_rows(H, W, perm, x_along).reshape(-1)      # the row of lattice point m W + n

    def _convolve(self, g, spectrum):
        H, W, nv = self.H, self.W, self.nv
        pad = np.zeros((2 * H, 2 * W, 2 * nv))
        pad[:H, :W, :nv] = g
        return np.fft.ifftn(np.fft.fftn(pad) * spectrum).real[:H, :W, :nv]

    def load_volume(self, volume):
        """g [H, W, nv]."""
        return np.asarray(volume, dtype=np.float64).transpose(2, 0, 1) @ self.R.T

    def store_rows(self, o):
        """rows [H W, nr] from the corner o [H, W, nv]."""
        rows = np.zeros((self.H * self.W, self.nr))
        rows[self.v] = ((o @ self.R) * self.w[None, None, :]).reshape(self.H * self.W, self.nr)
        return rows

    def load_rows(self, rows):
        """g [H, W, nv]."""
        psi = np.asarray(rows, dtype=np.float64)[self.v].reshape(self.H, self.W, self.nr) * self.w[None, None, :]
        return psi @ self.R.T

    def store_volume(self, o):
        """volume [W, nr, H] from the corner o [H, W, nv]."""
        return np.ascontiguousarray((o @ self.R).transpose(1, 2, 0))

    def forward(self, volume):
        return self.store_rows(self._convolve(self.load_volume(volume), self.Fk))

    def adjoint(self, rows):
        return self.store_volume(self._convolve(self.load_rows(rows), np.conj(self.Fk)))

    def norm(self, iterations=8):
        """The largest eigenvalue of A^T A by power iteration from ones, as LctOperator.norm."""
        v = np.ones((self.W, self.nr, self.H))
        lam = None
        for _ in range(iterations):
            v = v / np.sqrt((v * v).sum())
            v = self.adjoint(self.forward(v))
            lam = np.sqrt((v * v).sum())
        return float(lam)

    def solve(self, rows, iterations=30, nonneg=True, step=None, accelerate=False):
        """(volume, objective [iterations]) of lct_solve: projected Landweber, or FISTA with accelerate;
        objective[n] = 1/2 |A y_n - h|^2 where gradient n is taken."""
        h = np.asarray(rows, dtype=np.float64)
        step = 1.0 / self.norm() if step is None else float(step)
        x = np.zeros((self.W, self.nr, self.H))
        y, t = x.copy(), 1.0
        objective = np.zeros(iterations)
        for n in range(iterations):
            res = self.forward(y) - h
            objective[n] = 0.5 * (res * res).sum()
            xn = y - step * self.adjoint(res)
            if nonneg:
                xn = np.maximum(xn, 0.0)
            if accelerate:
                tn = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
                y = xn + ((t - 1.0) / tn) * (xn - x)
                t = tn
            else:
                y = xn
            x = xn
        return x, objective

    def objective(self, volume, rows):
        res = self.forward(volume) - np.asarray(rows, dtype=np.float64)
        return 0.5 * float((res * res).sum())


def project64(volume, H, W, sx, sz, r0, dr, power=0, nv=None, perm=None, x_along="n", R=None):
    """A volume: rows [H W, nr] float64."""
    nr = np.asarray(volume).shape[1]
    return Operator64(H, W, sx, sz, r0, dr, nr, power, nv, perm, x_along, R).forward(volume)


def adjoint64(rows, H, W, sx, sz, r0, dr, power=0, nv=None, perm=None, x_along="n", R=None):
    """A^T rows: a volume [W, nr, H] float64."""
    nr = np.asarray(rows).shape[1]
    return Operator64(H, W, sx, sz, r0, dr, nr, power, nv, perm, x_along, R).adjoint(rows)


def norm64(H, W, sx, sz, r0, dr, nr, power=0, nv=None, iterations=8):
    return Operator64(H, W, sx, sz, r0, dr, nr, power, nv).norm(iterations)


def solve64(rows, H, W, sx, sz, r0, dr, power=0, nv=None, iterations=30, nonneg=True, step=None, accelerate=False):
    nr = np.asarray(rows).shape[1]
    return Operator64(H, W, sx, sz, r0, dr, nr, power, nv).solve(rows, iterations, nonneg, step, accelerate)


def solver_rows(c):
    """(rows r^3 as fp32 [H W, nr], r0, dr) of a scatterer scene (fk_oracle.scatterer_scene): what the solver checks
    fit with power 0."""
    rows, xs, zs, r0, dr = FO.scatterer_scene(c)
    r = FO.f32(r0) + np.arange(c["nr"]) * FO.f32(dr)
    return (rows.astype(np.float64) * r[None, :] ** 3).astype(np.float32), r0, dr


@functools.lru_cache(maxsize=None)
def peak_solution(index):
    """The float64 solves of scene lct_oracle.PEAKS[index], computed once for all tests that need them:
    dict(case, rows, r0, dr, norm, landweber=(volume, objective), fista=(volume, objective), final=(1/2 |A x - h|^2
    of the two volumes)); 30 steps at step = 1 / norm, power 0."""
    name, nv, voxel = LO.PEAKS[index]
    c = LO.peak_case(name, voxel)
    rows, r0, dr = solver_rows(c)
    op = Operator64(c["H"], c["W"], c["sx"], c["sz"], r0, dr, c["nr"], 0, nv)
    norm = op.norm()
    lw = op.solve(rows, 30, step=1.0 / norm)
    fi = op.solve(rows, 30, step=1.0 / norm, accelerate=True)
    return dict(case=c, nv=nv, rows=rows, r0=r0, dr=dr, norm=norm, landweber=lw, fista=fi,
                final=(op.objective(lw[0], rows), op.objective(fi[0], rows)))


def blob(c, centre, std, xs, zs, r0, dr):
    """A Gaussian blob [W, nr, H] fp32 of standard deviation `std` around voxel `centre` of the lattice's grid."""
    n, j, m = centre
    ys = FO.f32(r0) + np.arange(c["nr"]) * FO.f32(dr)
    d2 = ((xs.astype(np.float64)[:, None, None] - float(xs[n])) ** 2 + (ys[None, :, None] - ys[j]) ** 2
          + (zs.astype(np.float64)[None, None, :] - float(zs[m])) ** 2)
    return np.exp(-0.5 * d2 / std ** 2).astype(np.float32)
