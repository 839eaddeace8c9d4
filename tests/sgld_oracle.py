"""float64 restatement of the SGLD noise step (nlosgr_sgld_noise, include/nlosgr.h) in numpy, from the fp32 inputs.

Philox4x32-10 on uint64 arrays (every product of two 32-bit words fits 64 bits), the open-interval uniforms
((x >> 9) + 0.5) 2^-23 (exact in fp32, so the kernel and this file share them bit for bit), Box-Muller, the
activations of both presets (nlosgr_device.hpp activate<PRESET>), the gate and Sigma xi = R'^T (s~^2 o (R' xi)).

The gate follows the header to the letter: where the kernel's fp32 expf(-gate_k a) overflows to inf
(exp > FLT_MAX) the gate is exactly 0; everywhere else it is 1 / (1 + exp(-gate_k a)) in float64.

reference() also returns, per Gaussian, the scale the parity rule judges against,
    s_g = scale gate max_r sum_c |Sigma_rc| |xi_c|.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
FLT_MAX = float(np.finfo(np.float32).max)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (32-bit words held in uint64 arrays, broadcast) -> words [..., 4] uint64."""
    counter = np.asarray(counter, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(counter[..., j], shape).copy() for j in range(4)]
    k = [np.broadcast_to(key[..., j], shape).copy() for j in range(2)]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> S32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return np.stack(c, axis=-1)


def words(seed, iteration, n):
    """The four words of elements n (array of indices) at `iteration` under `seed` (Python ints, 64 bits each)."""
    n = np.asarray(n, dtype=np.uint64)
    seed, iteration = int(seed) & (2 ** 64 - 1), int(iteration) & (2 ** 64 - 1)
    it = np.uint64(iteration)
    counter = np.stack([n & MASK, n >> S32, np.broadcast_to(it & MASK, n.shape), np.broadcast_to(it >> S32, n.shape)],
                       axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32_10(counter, key)


def uniforms(w):
    return ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(u):
    """u [..., 4] -> xi [..., 3] (Box-Muller, the kernel's pairing)."""
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    t0, t1 = 2.0 * np.pi * u[..., 1], 2.0 * np.pi * u[..., 3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=-1)


def xi_of(seed, iteration, n):
    return normals(uniforms(words(seed, iteration, n)))


def _quat_rot(q):
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def activation(scaling, rotation, preset, mod):
    """(s~ [N,3], R' [N,3,3]) of activate<PRESET>, float64 from the fp32 raw parameters."""
    S = np.asarray(scaling, dtype=np.float32).astype(np.float64)
    Q = np.asarray(rotation, dtype=np.float32).astype(np.float64)
    mod = float(np.float32(mod))
    with np.errstate(all="ignore"):
        n = np.sqrt((Q * Q).sum(1))
        if preset == "torch":
            st = np.exp(np.exp(S) * mod)
            qh = Q / np.maximum(n, 1e-12)[:, None]                 # F.normalize: a zero quaternion stays zero,
            Rp = _quat_rot(qh / np.sqrt((qh * qh).sum(1))[:, None])   # and build_rotation's own normalise makes it NaN
        elif preset == "cuda":
            st = np.exp(S) * mod + float(np.float32(1e-8))
            small = n < float(np.float32(1e-8))
            R = _quat_rot(Q / np.where(small, 1.0, n)[:, None])
            R[small] = np.eye(3)
            Rp = R.transpose(0, 2, 1)
        else:
            raise ValueError(preset)
    return st, Rp


def reference(scaling, rotation, opacity, preset, mod, seed, iteration, first_index, scale, gate_k=100.0,
              gate_x0=0.995):
    """dict: delta [N,3] (the noise added to mu), s [N] (the parity rule's scale), xi [N,3], u [N,4], gate [N]."""
    O = np.asarray(opacity, dtype=np.float32).astype(np.float64).reshape(-1)
    N = O.shape[0]
    scale, gate_k, gate_x0 = (float(np.float32(v)) for v in (scale, gate_k, gate_x0))
    u = uniforms(words(seed, iteration, int(first_index) + np.arange(N, dtype=np.uint64)))
    xi = normals(u)
    st, Rp = activation(scaling, rotation, preset, mod)
    with np.errstate(all="ignore"):
        sigma = 1.0 / (1.0 + np.exp(-O))
        a = (1.0 - sigma) - gate_x0
        e = np.exp(-gate_k * a)
        gate = np.where(e > FLT_MAX, 0.0, 1.0 / (1.0 + e))
        sxi = np.einsum("nrc,nr->nc", Rp, st * st * np.einsum("nrc,nc->nr", Rp, xi))
        Sigma = np.einsum("nra,nr,nrb->nab", Rp, st * st, Rp)
        delta = (scale * gate)[:, None] * sxi
        s = scale * gate * (np.abs(Sigma) * np.abs(xi)[:, None, :]).sum(2).max(1)
    return dict(delta=delta, s=s, xi=xi, u=u, gate=gate, sigma_xi=sxi)
