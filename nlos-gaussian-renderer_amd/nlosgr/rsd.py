"""Fast phasor-field reconstruction: the phasor field evaluated as Rayleigh-Sommerfeld diffraction, RSD (Liu, Bauer,
Velten 2020), by FFT on the wall's lattice.  Where nlosgr.phasor visits every (voxel, measurement) pair, O(N^5), this
is O(N^3 log N) per frequency of the wavelet's band: for one depth plane and one temporal frequency the sum over the
wall points is a 2-D convolution over the lattice.  It serves a confocal capture and the most common non-confocal
one, a fixed laser spot with a scanned sensor lattice; the weight (|x - laser| |x - wall|)^(power/2) of
backproject(..., lasers=) separates into a laser and a sensor factor, so this computes the quantity the project
already defines.  The volume's x and z are the wall lattice's own; its depths are free (include/nlosgr.h states every
formula):

    rows [H W, nr] -> S = rfft(rows, Nt)                                                    torch.fft
                   -> Pw[q] = coef[q] S[., q] as zero-padded images [nq, 2H, 2W]             nlosgr_rsd_load
                   -> Pf = fft2(Pw)                                                          torch.fft
    per chunk of depth planes:
                   -> K[j, q] = d^e exp(2 pi i g q (d / dr) / Nt) over the signed offsets    nlosgr_rsd_kernel
                   -> Kf = fft2(K);  Kf *= Pf;  o = ifft2(Kf)                                torch.fft, nlosgr_rsd_apply
                   -> Phi[n, j, m] = sum_q L_q o[j, q, m, n], planes and magnitude           nlosgr_rsd_gather

Against phasor_backproject there is no linear interpolation between bins, no +-3 sigma truncation of the wavelet's
taps, the band is cut at +-3 sigma_q, and the filtered rows are periodic in Nt (rsd_nt picks an Nt at which nothing
wraps).  Bitwise repeatable; the rows may be in any order (perm=).  Per-measurement laser spots go to nlosgr.phasor.

No CPU fallback, no backward.

    python -m nlosgr.rsd CAPTURE.mat --resolution R --start S --end E --wavelength L [--cycles C] [--power P]
        --out rsd.npz [--mesh rsd.ply --level-frac F]
"""
import math

import numpy as np
import torch

from . import _cli, _lib
from .lattice import _f32, _gpu, _work, capture_lattice, capture_result, lattice_rows, lattice_spacing
from .voxelize import MAX_EXTENT, VoxelGrid

MAX_NT = 8192
MAX_BAND = 512


def rsd_band(wavelength, dr, Nt, r0, cycles=4.0):
    """(q_lo, coef): the first DFT bin of the wavelet's band and its complex128 coefficients [nq], built in double
    from the fp32 values of r0 and dr.  P = wavelength / (2 dr) bins per period, sigma_b = cycles P / 6,
    theta_q = 2 pi q / Nt, theta_0 = 2 pi / P, q_0 = Nt / P, sigma_q = Nt / (2 pi sigma_b); the band is
    [max(1, ceil(q_0 - 3 sigma_q)), min(Nt/2 - 1, floor(q_0 + 3 sigma_q))] and
    coef[q] = exp(-(sigma_b (theta_q - theta_0))^2 / 2) exp(-i theta_q r0 / dr) / Nt.  ValueError for P < 2,
    cycles <= 0, r0 < 0, an Nt that is odd or outside 2..8192, an empty band or one of more than 512 bins."""
    wavelength, cycles, dr, r0, Nt = float(wavelength), float(cycles), _f32(dr), _f32(r0), int(Nt)
    if not (dr > 0 and math.isfinite(dr)):
        raise ValueError("nlosgr: dr must be finite and > 0")
    if not (r0 >= 0 and math.isfinite(r0)):
        raise ValueError("nlosgr: r0 must be finite and >= 0")
    if not cycles > 0:
        raise ValueError("nlosgr: cycles must be > 0")
    if Nt % 2 or not 2 <= Nt <= MAX_NT:
        raise ValueError(f"nlosgr: Nt must be even and in 2..{MAX_NT}")
    P = wavelength / (2.0 * dr)
    if not P >= 2.0:
        raise ValueError(f"nlosgr: wavelength {wavelength} is {P:.3g} bins per period; the rows resolve >= 2 (Nyquist)")
    sigma_b = cycles * P / 6.0
    q0, sigma_q = Nt / P, Nt / (2.0 * math.pi * sigma_b)
    q_lo = max(1, int(math.ceil(q0 - 3.0 * sigma_q)))
    q_hi = min(Nt // 2 - 1, int(math.floor(q0 + 3.0 * sigma_q)))
    nq = q_hi - q_lo + 1
    if nq < 1:
        raise ValueError("nlosgr: the wavelet's band holds no DFT bin of 1..Nt/2 - 1 (raise Nt or the wavelength)")
    if nq > MAX_BAND:
        raise ValueError(f"nlosgr: the wavelet's band holds {nq} DFT bins (> {MAX_BAND}); raise cycles or the wavelength")
    theta = 2.0 * math.pi * np.arange(q_lo, q_hi + 1, dtype=np.float64) / Nt
    coef = np.exp(-0.5 * (sigma_b * (theta - 2.0 * math.pi / P)) ** 2) * np.exp(-1j * theta * (r0 / dr)) / Nt
    return q_lo, coef


def _smooth_even(n):
    """The smallest even 2^a 3^b 5^c >= n."""
    n = max(int(n), 2)
    best = None
    p5 = 1
    while p5 < 2 * n:
        p3 = p5
        while p3 < 2 * n:
            v = 2 * p3
            while v < n:
                v *= 2
            if best is None or v < best:
                best = v
            p3 *= 3
        p5 *= 5
    return best


def rsd_nt(nr, xs, zs, y0, ys, r0, dr, wavelength, cycles=4.0, laser=None):
    """The default DFT length: the smallest even 2^a 3^b 5^c that is at least
    max(t_max, nr) - min(t_min, 0) + ceil(4 sigma_b) + 1, so that no pair's bin coordinate, with the wavelet's reach,
    wraps onto the data.  t_max: the largest bin coordinate (u - r0) / dr over the voxel box's 8 corners x the wall's
    4 corners (u, the half path, is jointly convex in the two points, so the corners bound it from above); t_min:
    the coordinate of the smallest conceivable half path, the first depth (with a laser, the mean of it and the
    laser's distance to the depth range).  ValueError when that exceeds 8192."""
    f = lambda t: np.asarray(torch.as_tensor(t).detach().cpu(), dtype=np.float64).reshape(-1)
    xs, ys, zs = f(xs), f(ys), f(zs)
    dr, r0, y0 = _f32(dr), _f32(r0), float(y0)
    sigma_b = float(cycles) * (float(wavelength) / (2.0 * dr)) / 6.0
    box = np.array([(x, y, z) for x in (xs[0], xs[-1]) for y in (ys[0], ys[-1]) for z in (zs[0], zs[-1])])
    wall = np.array([(x, y0, z) for x in (xs[0], xs[-1]) for z in (zs[0], zs[-1])])
    u = np.sqrt(((box[:, None, :] - wall[None, :, :]) ** 2).sum(axis=2))
    u_min = ys[0] - y0
    if laser is not None:
        l = np.asarray([float(v) for v in laser], dtype=np.float64)
        u = 0.5 * (u + np.sqrt(((box - l[None]) ** 2).sum(axis=1))[:, None])
        u_min = 0.5 * (u_min + max(ys[0] - l[1], l[1] - ys[-1], 0.0))
    t_max, t_min = (float(u.max()) - r0) / dr, (float(u_min) - r0) / dr
    need = max(t_max, float(nr)) - min(t_min, 0.0) + math.ceil(4.0 * sigma_b) + 1
    Nt = _smooth_even(int(math.ceil(need)))
    if Nt > MAX_NT:
        raise ValueError(f"nlosgr: this reconstruction needs a DFT length of {Nt} (> {MAX_NT}); move the window "
                         "(start / end) nearer to the volume or shorten the wavelet")
    return Nt


def _lattice(H, W):
    H, W = int(H), int(W)
    if not (1 <= H <= MAX_EXTENT and 1 <= W <= MAX_EXTENT):
        raise ValueError(f"nlosgr: RSD lattice extents H, W must be in 1..{MAX_EXTENT}")
    return H, W


def _depths(ys, y0, what):
    """ys as a contiguous fp32 GPU table [ny] with every depth ys[j] - y0 finite and > 0 (read back and checked)."""
    ys = _gpu(ys, torch.float32, what)
    if ys.dim() != 1 or not 1 <= ys.shape[0] <= MAX_EXTENT:
        raise ValueError(f"nlosgr: ys must be a table of 1..{MAX_EXTENT} depths")
    D = ys.double().cpu().numpy() - float(np.float32(y0))
    if not (np.isfinite(D).all() and (D > 0).all()):
        raise ValueError("nlosgr: every depth ys[j] - y0 must be finite and > 0 (the volume lies in front of the wall)")
    return ys


def _chunk(ny, j0, nj):
    j0 = int(j0)
    nj = ny - j0 if nj is None else int(nj)
    if j0 < 0 or nj < 1 or j0 + nj > ny:
        raise ValueError(f"nlosgr: depth planes [{j0}, {j0 + nj}) outside the table's {ny}")
    return j0, nj


@torch.no_grad()
def rsd_load(spec, H, W, q_lo, coef, perm=None, x_along="n", out=None):
    """Stage 2, complex64 [nq, 2H, 2W]: the band of spec = rfft(rows, Nt) ([H W, Nt/2 + 1]) times coef (rsd_band), as
    zero-padded frequency-major images (nlosgr_rsd_load; every element of `out` is written).  perm: int32 [H W],
    the row that holds lattice point v (None: row v)."""
    lib = _lib.load()
    spec = _gpu(spec, torch.complex64, "rsd_load")
    H, W = _lattice(H, W)
    if spec.dim() != 2 or spec.shape[0] != H * W or spec.shape[1] < 2:
        raise ValueError(f"nlosgr: rsd_load takes a spectrum [{H * W}, Nt/2 + 1] for an {H} x {W} lattice")
    dev = spec.device
    Nt = 2 * (int(spec.shape[1]) - 1)
    coef = torch.as_tensor(coef).to(device=dev, dtype=torch.complex64).reshape(-1).contiguous()
    nq, q_lo = int(coef.shape[0]), int(q_lo)
    if not (1 <= nq <= MAX_BAND and q_lo >= 1 and q_lo + nq - 1 <= Nt // 2 - 1):
        raise ValueError(f"nlosgr: the band [q_lo, q_lo + nq) must lie in [1, Nt/2 - 1] and hold 1..{MAX_BAND} bins")
    perm, sm, sn = lattice_rows(perm, x_along, H, W, dev, "rsd_load")
    pw = _work(out, (nq, 2 * H, 2 * W), dev, "rsd_load")
    _lib.check(lib.nlosgr_rsd_load(_lib.ptr(spec), _lib.ptr(perm), _lib.ptr(coef), H, W, Nt, q_lo, nq, sm, sn,
                                   _lib.ptr(pw), _lib.stream_handle(dev)))
    return pw


@torch.no_grad()
def rsd_kernel(ys, y0, H, W, sx, sz, dr, Nt, q_lo, nq, power=0, laser=False, j0=0, nj=None, out=None):
    """Stage 5, complex64 [nj, nq, 2H, 2W]: the diffraction kernels of depth planes [j0, j0 + nj) of the fp32 GPU
    table ys over the signed lattice offsets (nlosgr_rsd_kernel; every element of `out` is written, the entries at
    offset -H or -W with zero).  laser: the half-weight, half-phase form of a capture with one laser spot."""
    lib = _lib.load()
    ys = _depths(ys, y0, "rsd_kernel")
    H, W = _lattice(H, W)
    j0, nj = _chunk(int(ys.shape[0]), j0, nj)
    if not (float(sx) > 0 and float(sz) > 0 and float(dr) > 0):
        raise ValueError("nlosgr: sx, sz and dr must be > 0")
    K = _work(out, (nj, int(nq), 2 * H, 2 * W), ys.device, "rsd_kernel")
    _lib.check(lib.nlosgr_rsd_kernel(_lib.ptr(ys), int(ys.shape[0]), j0, nj, float(y0), H, W, float(sx), float(sz),
                                     float(dr), int(Nt), int(q_lo), int(nq), int(power), int(bool(laser)),
                                     _lib.ptr(K), _lib.stream_handle(ys.device)))
    return K


@torch.no_grad()
def rsd_apply(Kf, Pf, out=None):
    """Stage 7, complex64 [nj, nq, 2H, 2W]: Kf[j, q] Pf[q], broadcast over j (nlosgr_rsd_apply).  out=None works in
    place and returns Kf; another `out` must not overlap either input."""
    lib = _lib.load()
    Pf = _gpu(Pf, torch.complex64, "rsd_apply")
    if isinstance(Kf, torch.Tensor) and not Kf.is_contiguous():       # (a copy would be filled, not the caller's)
        raise ValueError("nlosgr: rsd_apply works in place on a contiguous complex64 [nj, nq, 2H, 2W] tensor")
    Kf = _gpu(Kf, torch.complex64, "rsd_apply")
    if (Kf.dim() != 4 or Pf.dim() != 3 or tuple(Kf.shape[1:]) != tuple(Pf.shape) or Kf.device != Pf.device
            or Kf.shape[2] % 2 or Kf.shape[3] % 2):
        raise ValueError("nlosgr: rsd_apply takes Kf [nj, nq, 2H, 2W] and Pf [nq, 2H, 2W] on one device")
    nj, nq, H, W = int(Kf.shape[0]), int(Kf.shape[1]), int(Kf.shape[2]) // 2, int(Kf.shape[3]) // 2
    _lattice(H, W)
    out = Kf if out is None else _work(out, Kf.shape, Kf.device, "rsd_apply")
    _lib.check(lib.nlosgr_rsd_apply(_lib.ptr(Kf), _lib.ptr(Pf), nj, nq, H, W, _lib.ptr(out),
                                    _lib.stream_handle(Kf.device)))
    return out


def _laser(laser):
    if laser is None:
        return None
    l = [_f32(v) for v in torch.as_tensor(laser).detach().cpu().reshape(-1).tolist()]
    if len(l) != 3 or not all(math.isfinite(v) for v in l):
        raise ValueError("nlosgr: laser must be one finite point [3] (per-measurement spots: nlosgr.phasor)")
    return l


@torch.no_grad()
def rsd_gather(field, q_lo, Nt, dr, xs, ys, zs, power=0, laser=None, j0=0, out=None, mag=None):
    """Stage 9, (planes [2, W, ny, H], mag [W, ny, H]) fp32: the sum over the band of field [nj, nq, 2H, 2W] =
    ifft2(rsd_apply(...)) on its [0:H, 0:W] corner, with the laser's factor when `laser` [3] is given, written to depth
    planes [j0, j0 + nj) of `out` and `mag` in the voxel order (nlosgr_rsd_gather).  xs [W], ys [ny], zs [H]: fp32 GPU
    tables.  out / mag: tensors to write into (the other planes are left as they are); None: new ones, whose other
    planes are uninitialised."""
    lib = _lib.load()
    field = _gpu(field, torch.complex64, "rsd_gather")
    if field.dim() != 4 or field.shape[2] % 2 or field.shape[3] % 2:
        raise ValueError("nlosgr: rsd_gather takes a field [nj, nq, 2H, 2W]")
    nj, nq = int(field.shape[0]), int(field.shape[1])
    H, W = _lattice(int(field.shape[2]) // 2, int(field.shape[3]) // 2)
    dev = field.device
    xs, ys, zs = (_gpu(t, torch.float32, "rsd_gather") for t in (xs, ys, zs))
    if xs.shape != (W,) or zs.shape != (H,) or ys.dim() != 1 or not 1 <= ys.shape[0] <= MAX_EXTENT:
        raise ValueError(f"nlosgr: rsd_gather takes tables xs [{W}], ys [1..{MAX_EXTENT}], zs [{H}]")
    ny = int(ys.shape[0])
    j0, nj = _chunk(ny, j0, nj)
    if not float(dr) > 0:
        raise ValueError("nlosgr: dr must be > 0")
    res = []
    for t, shape in ((out, (2, W, ny, H)), (mag, (W, ny, H))):
        if t is None:
            t = torch.empty(shape, dtype=torch.float32, device=dev)
        elif (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("nlosgr: rsd_gather needs float32 GPU tensors (no CPU fallback)")
        elif tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"nlosgr: out / mag must be a contiguous float32 {shape} tensor on {dev}")
        res.append(t)
    planes, mag = res
    l = _laser(laser)
    _lib.check(lib.nlosgr_rsd_gather(_lib.ptr(field), H, W, nq, int(q_lo), int(Nt), float(dr), int(power),
                                     _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(zs), ny, j0, nj, int(l is not None),
                                     *(l or (0.0, 0.0, 0.0)), _lib.ptr(planes), _lib.ptr(mag),
                                     _lib.stream_handle(dev)))
    return planes, mag


@torch.no_grad()
def rsd_reconstruct(rows, H, W, xs, zs, y0, ys, r0, dr, wavelength, cycles=4.0, power=0, laser=None, perm=None,
                    x_along="n", Nt=None, work_bytes=1 << 30):
    """(planes [2, W, ny, H], mag [W, ny, H]) fp32: the phasor field of rows [H W, nr] (float32, GPU), the row of
    lattice point v = m W + n (x_along="n") or v = n H + m ("m") being rows[perm[v]] (perm None: rows[v]), measured at
    (xs[n], y0, zs[m]) (uniform fp32 tables), at the voxels (xs[n], ys[j], zs[m]): ys is an ascending fp32 table of any
    spacing with ys[j] > y0.  r0: radius of bin 0; dr: bin width; wavelength, cycles: as phasor_kernel; power 0..4: the
    weight of backproject; laser: one spot [3], or None for a confocal capture.  Nt: the even DFT length, nr <= Nt <=
    8192 (None: rsd_nt; a larger one is always allowed).  The depth planes are done in chunks whose two work arrays
    stay within work_bytes each (at least one plane per chunk)."""
    rows = _gpu(rows, torch.float32, "rsd_reconstruct")
    H, W = _lattice(H, W)
    if rows.dim() != 2 or rows.shape[0] != H * W or rows.shape[1] < 1:
        raise ValueError(f"nlosgr: rows must be [{H * W}, nr] for an {H} x {W} lattice")
    dev, nr = rows.device, int(rows.shape[1])
    if not 0 <= int(power) <= 4:
        raise ValueError("nlosgr: power must be in 0..4")
    f32t = lambda t: torch.as_tensor(t).detach().to(torch.float32).reshape(-1)
    xs, zs, ys = f32t(xs), f32t(zs), f32t(ys)
    if xs.shape[0] != W or zs.shape[0] != H:
        raise ValueError(f"nlosgr: xs must be [{W}] and zs [{H}]")
    sx = lattice_spacing(xs.cpu(), None if W > 1 else lattice_spacing(zs.cpu()))
    sz = lattice_spacing(zs.cpu(), sx)
    if not (sx > 0 and sz > 0):
        raise ValueError("nlosgr: xs and zs must ascend")
    xs, zs = xs.to(dev).contiguous(), zs.to(dev).contiguous()
    ys = _depths(ys.to(dev), y0, "rsd_reconstruct")
    ny = int(ys.shape[0])
    l = _laser(laser)
    if Nt is None:
        Nt = rsd_nt(nr, xs, zs, y0, ys, r0, dr, wavelength, cycles, l)
    Nt = int(Nt)
    if Nt % 2 or not nr <= Nt <= MAX_NT:
        raise ValueError(f"nlosgr: Nt must be even and in nr..{MAX_NT}")
    q_lo, coef = rsd_band(wavelength, dr, Nt, r0, cycles)
    nq = len(coef)
    Pf = torch.fft.fft2(rsd_load(torch.fft.rfft(rows, n=Nt), H, W, q_lo, coef, perm=perm, x_along=x_along))
    per_plane = nq * 4 * H * W * 8
    step = min(ny, max(1, int(work_bytes) // per_plane))
    A = torch.empty((step, nq, 2 * H, 2 * W), dtype=torch.complex64, device=dev)
    B = torch.empty_like(A)
    planes = torch.empty((2, W, ny, H), dtype=torch.float32, device=dev)
    mag = torch.empty((W, ny, H), dtype=torch.float32, device=dev)
    for j0 in range(0, ny, step):
        nj = min(step, ny - j0)
        a, b = A[:nj], B[:nj]
        rsd_kernel(ys, y0, H, W, sx, sz, dr, Nt, q_lo, nq, power=power, laser=l is not None, j0=j0, nj=nj, out=a)
        torch.fft.fft2(a, out=b)
        rsd_apply(b, Pf)
        torch.fft.ifft2(b, out=a)
        rsd_gather(a, q_lo, Nt, dr, xs, ys, zs, power=power, laser=l, j0=j0, out=planes, mag=mag)
    return planes, mag


def capture_laser(data_kwargs):
    """The one laser spot [3] of the capture in data_kwargs, or None for a confocal capture (no laser key, or spots
    equal to the sensed points).  NotImplementedError when the spots differ from measurement to measurement."""
    from .data import is_confocal
    if is_confocal(data_kwargs):
        return None
    lasers = data_kwargs["laser_grid_positions"].detach().float().cpu()
    if lasers.dim() == 2 and lasers.shape[0] == 3 and bool((lasers == lasers[:, :1]).all()):
        return [float(v) for v in lasers[:, 0]]
    raise NotImplementedError("nlosgr: the fast phasor field takes a confocal capture or one laser spot for the whole "
                              "capture: this capture's laser spots (laser_grid_positions) differ from measurement to "
                              "measurement.  Use nlosgr.phasor, which takes them")


@torch.no_grad()
def rsd_capture(data_kwargs, resolution, start, end, wavelength, cycles=4.0, power=0, crop=True):
    """Fast phasor-field image of the capture in data_kwargs (data.make_data_kwargs, shuffled or not) over bins
    [floor(start), floor(start) + end - start): x and z are the wall lattice's own (lattice.wall_lattice), the depths
    the y table of VoxelGrid(volume_position, volume_size, resolution), as phasor_capture's.  crop: keep the lattice
    points inside the capture's volume box, a contiguous block, as fk_capture does.  A capture with one laser spot (a
    [3, 1] field, or all spots equal) is reconstructed with it; distinct spots raise NotImplementedError.  Returns
    the keys of phasor_capture: {"volume" (the magnitude), "real", "imag", "front", "depth", "grid"}."""
    laser = capture_laser(data_kwargs)
    c = capture_lattice(data_kwargs, start, end, extents=False)
    vp = [float(v) for v in data_kwargs["volume_position"]]
    ys = VoxelGrid(vp, float(data_kwargs["volume_size"]), resolution).ys
    planes, mag = rsd_reconstruct(c.rows, c.H, c.W, c.xs, c.zs, c.y0, ys, c.r0, c.dr, wavelength, cycles=cycles,
                                  power=power, laser=laser, perm=c.perm, x_along=c.x_along)
    return capture_result(data_kwargs, VoxelGrid(tables=(c.xs, ys, c.zs)), mag, crop, axes=(0, 2), real=planes[0],
                          imag=planes[1])


def parse_args(argv=None):
    ap = _cli.capture_parser("python -m nlosgr.rsd", "rsd.npz",
                             "Fast phasor-field reconstruction (Rayleigh-Sommerfeld diffraction by FFT) of a confocal "
                             "capture or one with a single laser spot, on the wall's lattice x the volume's depths.")
    ap.add_argument("--resolution", type=int, default=128, help="depth planes across the volume box")
    ap.add_argument("--wavelength", type=float, required=True,
                    help="virtual wavelength in scene units along the whole path (2-4 wall-point spacings or more)")
    ap.add_argument("--cycles", type=float, default=4.0, help="periods inside +-3 sigma of the envelope")
    ap.add_argument("--power", type=int, default=0, choices=range(5), help="weight d^power")
    return _cli.parse(ap, argv)


def main(argv=None):
    a = parse_args(argv)
    dk = _cli.open_capture(a.capture, "the fast phasor field")
    out = rsd_capture(dk, a.resolution, a.start, a.end, a.wavelength, cycles=a.cycles, power=a.power)
    _cli.write_volume(a, dk, out, f"wavelength {a.wavelength}, cycles {a.cycles}, power {a.power}",
                      real=out["real"].cpu().numpy(), imag=out["imag"].cpu().numpy())


if __name__ == "__main__":
    main()
