"""One SHA-256 per case of the raw output bytes of the reconstructions on the wall's lattice (nlosgr.fk, nlosgr.lct,
nlosgr.rsd) and of the six capture command lines, from seeded inputs.  A refactor must leave every digest as it was:

    python scripts/lattice_digests.py --tree PARENT_CHECKOUT > before.txt
    python scripts/lattice_digests.py > after.txt && cmp before.txt after.txt

(one process per tree; --tree: the checkout whose nlosgr package, built library and tests/ are used, default this
one).  Cases: every stage function, the end-to-end calls and LctOperator on lattices 1x1, 1x5, 4x6, 3x65, 65x2 (and
6x3 for the 8-byte store) x 1, 2, 7, 8, 65, 130 bins, rows with negative entries and one NaN bin, rows offset by one
float, every power each entry point takes, amplitude on and off, x_along "n" and "m", perm None and a seeded
permutation, nv in {1, nr, 2 nr + 1}; RSD with a band of 123 frequencies, without and with a laser spot, and one
plane per chunk; the oracles' dense cases; the four *_capture functions on a synthetic capture, shuffled and not,
cropped and not; the six command lines (the arrays of the npz, key by key, and the printed lines).  A case that
raises is hashed over the exception's class and text.

    python scripts/lattice_digests.py --host-only [--tree ...]

needs no GPU: it replays test_entry_points_validate_on_the_host of the four tests/test_{fk,lct,lct_op,rsd}_cpu.py
and hashes the status and nlosgr_last_error() of every nlosgr_fk_* / nlosgr_lct_* / nlosgr_rsd_* call they make.
"""
import argparse
import contextlib
import hashlib
import importlib
import io
import os
import sys
import tempfile

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--host-only", action="store_true")
ARGS = ap.parse_args()
TREE = os.path.abspath(ARGS.tree)
sys.path[:0] = [os.path.join(TREE, "nlos-gaussian-renderer_amd"), os.path.join(TREE, "tests")]
import torch  # noqa: E402

import fk_oracle as FO  # noqa: E402
import rsd_oracle as RO  # noqa: E402
_lib, backproject, fk, forward_project, lct, phasor, rsd = (
    importlib.import_module("nlosgr." + m) for m in ("_lib", "backproject", "fk", "forward_project", "lct", "phasor", "rsd"))

DEV = "cuda:0"
COUNT = 0
LATTICES = ((1, 1), (1, 5), (4, 6), (3, 65), (65, 2))
BINS = (1, 2, 7, 8, 65, 130)
SX, SZ, R0, DR = 0.05, 0.07, 0.06, 0.02


def emit(name, fn):
    """Hash what fn() returns: tensors, arrays, strings, and tuples / dicts of them (a VoxelGrid: its tables)."""
    global COUNT
    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, torch.Tensor):
            h.update(v.detach().cpu().contiguous().numpy().tobytes())
        elif isinstance(v, np.ndarray):
            h.update(str(v.dtype).encode() + np.ascontiguousarray(v).tobytes())
        elif isinstance(v, (str, bytes, int)):
            h.update(v if isinstance(v, bytes) else str(v).encode())
        elif isinstance(v, dict):
            for k in sorted(v):
                feed(k), feed(v[k])
        elif hasattr(v, "tables"):
            feed(tuple(v.tables))
        else:
            for x in v:
                feed(x)

    try:
        feed(fn())
        what = ""
    except Exception as e:  # noqa: BLE001  (the refusals are cases too)
        feed(f"{type(e).__name__}: {e}")
        what = f" raised {type(e).__name__}"
    print(name, h.hexdigest() + what, flush=True)
    COUNT += 1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host_only():
    import test_fk_cpu, test_lct_cpu, test_lct_op_cpu, test_rsd_cpu  # noqa: E401
    lib = _lib.load()

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith(("nlosgr_fk_", "nlosgr_lct_", "nlosgr_rsd_")):
                return fn

            def call(*a):
                status = fn(*a)
                emit(f"host {name} #{COUNT}", lambda: (status, lib.nlosgr_last_error()))
                return status
            return call

    load, _lib.load = _lib.load, lambda: Recorder()
    try:
        for mod in (test_fk_cpu, test_lct_cpu, test_lct_op_cpu, test_rsd_cpu):
            mod.test_entry_points_validate_on_the_host()
    finally:
        _lib.load = load


def rows_of(g, H, W, nr):
    rows = g.random((H * W, nr), dtype=np.float32) + 0.05
    neg = g.random(rows.shape) < 0.05
    rows[neg] = -rows[neg]
    rows[(H * W) // 2, nr // 2] = np.nan
    return rows


def cplx(g, shape):
    return dev((g.standard_normal(shape) + 1j * g.standard_normal(shape)).astype(np.complex64))


def fk_cases(tag, g, H, W, nr, rows, orders):
    for p in range(5):
        for amp in (True, False):
            emit(f"fk_load {tag} p{p} amp{int(amp)}", lambda: fk.fk_load(rows, H, W, R0, DR, power=p, amplitude=amp))
    for name, kw in orders.items():
        emit(f"fk_load {tag} {name}", lambda: fk.fk_load(rows, H, W, R0, DR, **kw))
        emit(f"fk_migrate {tag} {name}", lambda: fk.fk_migrate(rows.nan_to_num(), H, W, SX, SZ, R0, DR, **kw))
    shifted = torch.empty(H * W * nr + 1, device=DEV)[1:].view(H * W, nr).copy_(rows)   # 4 bytes off the alignment
    emit(f"fk_load {tag} offset", lambda: fk.fk_load(shifted, H, W, R0, DR))
    emit(f"fk_stolt {tag}", lambda: fk.fk_stolt(cplx(g, (2 * H, 2 * W, 2 * nr)), SX, SZ, R0, DR))
    emit(f"fk_store {tag}", lambda: fk.fk_store(cplx(g, (2 * H, 2 * W, 2 * nr))))


def lct_cases(tag, g, H, W, nr, nv, rows, orders):
    tag = f"{tag} nv{nv}"
    res = lct.lct_resampling(R0, DR, nr, nv)
    field, vol = cplx(g, (2 * H, 2 * W, 2 * nv)), dev(g.standard_normal((W, nr, H)).astype(np.float32))
    for p in range(5):
        emit(f"lct_load {tag} p{p}", lambda: lct.lct_load(rows, H, W, R0, DR, power=p, nv=nv))
    for p in range(-4, 5):
        emit(f"lct_load_rows {tag} p{p}", lambda: lct.lct_load_rows(rows, H, W, R0, DR, power=p, nv=nv))
        emit(f"lct_store_rows {tag} p{p}", lambda: lct.lct_store_rows(field, res, power=p))
    for name, kw in orders.items():
        emit(f"lct_load {tag} {name}", lambda: lct.lct_load(rows, H, W, R0, DR, nv=nv, **kw))
        emit(f"lct_load_rows {tag} {name}", lambda: lct.lct_load_rows(rows, H, W, R0, DR, power=-2, nv=nv, **kw))
        emit(f"lct_store_rows {tag} {name}", lambda: lct.lct_store_rows(field, res, power=-2, **kw))
        emit(f"lct_reconstruct {tag} {name}", lambda: lct.lct_reconstruct(rows.nan_to_num(), H, W, SX, SZ, R0, DR,
                                                                            nv=nv, **kw))
        for p in (-3, 0, 2):
            op = lambda: lct.LctOperator(H, W, SX, SZ, R0, DR, nr, power=p, nv=nv, device=DEV, **kw)
            emit(f"LctOperator.forward {tag} {name} p{p}", lambda: op().forward(vol))
            emit(f"LctOperator.adjoint {tag} {name} p{p}", lambda: op().adjoint(rows.nan_to_num()))
    emit(f"lct_store {tag}", lambda: lct.lct_store(field, res))
    emit(f"lct_store_volume {tag}", lambda: lct.lct_store_volume(field, res))
    emit(f"lct_load_volume {tag}", lambda: lct.lct_load_volume(vol, res))
    emit(f"lct_kernel {tag}", lambda: lct.lct_kernel(H, W, nv, SX, SZ, res.dv, device=DEV))
    for kw in (dict(snr=0.8), dict(backprop=True)):
        emit(f"lct_filter {tag} {kw}", lambda: lct.lct_filter(field, kf=field.flip(0), **kw))
        emit(f"lct_inverse {tag} {kw}", lambda: lct.lct_inverse(H, W, nv, SX, SZ, res.dv, kw.get("snr", 1.0),
                                                                 backprop="backprop" in kw, device=DEV))
    emit(f"lct_filter {tag} given", lambda: lct.lct_filter(field, inverse=field.flip(0)))


def rsd_cases(tag, g, H, W, nr, rows, orders):
    Nt, q_lo, nq = 256, 5, 40                                      # a band of more than one 32-tile
    xs, zs, _ = FO.lattice(H, W, SX, SZ)
    ys = np.array([0.3, 0.41, 0.55], dtype=np.float32)
    laser = (0.11, 0.0, -0.07)
    spec, coef = cplx(g, (H * W, Nt // 2 + 1)), cplx(g, (nq,))
    for name, kw in orders.items():
        emit(f"rsd_load {tag} {name}", lambda: rsd.rsd_load(spec, H, W, q_lo, coef, **kw))
        for las in (None, laser):
            for wb in (1 << 30, 1):
                emit(f"rsd_reconstruct {tag} {name} laser{int(las is not None)} wb{wb}",
                     lambda: rsd.rsd_reconstruct(rows.nan_to_num(), H, W, xs, zs, 0.0, ys, R0, DR, 16 * DR, cycles=1.0,
                                                 power=2, laser=las, Nt=Nt, work_bytes=wb, **kw))
    K = cplx(g, (3, nq, 2 * H, 2 * W))
    for p in range(5):
        for las in (False, True):
            emit(f"rsd_kernel {tag} p{p} laser{int(las)}",
                 lambda: rsd.rsd_kernel(dev(ys), 0.0, H, W, SX, SZ, DR, Nt, q_lo, nq, power=p, laser=las))
        for las in (None, laser):
            emit(f"rsd_gather {tag} p{p} laser{int(las is not None)}",
                 lambda: rsd.rsd_gather(K, q_lo, Nt, DR, dev(xs), dev(ys), dev(zs), power=p, laser=las))
    emit(f"rsd_apply {tag}", lambda: rsd.rsd_apply(K.clone(), cplx(g, (nq, 2 * H, 2 * W))))


def stages():
    for H, W in LATTICES + ((6, 3),):
        for nr in BINS if (H, W) != (6, 3) else (8,):
            g = np.random.default_rng(1000 * H + 10 * W + nr)
            tag = f"{H}x{W}x{nr}"
            rows = dev(rows_of(g, H, W, nr))
            perm = dev(g.permutation(H * W).astype(np.int32))
            orders = {"n": {}, "n-perm": dict(perm=perm), "m": dict(x_along="m"), "m-perm": dict(perm=perm, x_along="m")}
            fk_cases(tag, g, H, W, nr, rows, orders)
            for nv in sorted({1, nr, 2 * nr + 1}) if (H, W) in ((4, 6), (3, 65)) else (nr,):
                lct_cases(tag, g, H, W, nr, nv, rows, orders)
            if nr in (8, 65, 130):
                rsd_cases(tag, g, H, W, nr, rows, orders)


def dense():
    for name, c in FO.DENSE.items():
        rows, (r0, dr) = dev(FO.dense_rows(c)), FO.window(c)
        a = (rows, c["H"], c["W"], c["sx"], c["sz"], r0, dr)
        emit(f"dense fk_migrate {name}", lambda: fk.fk_migrate(*a))
        emit(f"dense lct_reconstruct {name}", lambda: lct.lct_reconstruct(*a))
        emit(f"dense lct_adjoint {name}", lambda: lct.lct_adjoint(*a, power=-1))
        emit(f"dense lct_project {name}", lambda: lct.lct_project(lct.lct_adjoint(*a), *a[1:], power=-1))
    for name in RO.DENSE:
        kw, laser = RO.dense_problem(name)
        kw["rows"] = dev(kw["rows"])
        for las in (None, laser):
            emit(f"dense rsd_reconstruct {name} laser{int(las is not None)}",
                 lambda: rsd.rsd_reconstruct(power=2, laser=las, **kw))


def write_capture(path, lasers):
    """The r0 = 20 dr scatterer of the GPU tests as a capture file: 84 bins of a 16 x 16 wall, window [20, 84)."""
    from nlosgr.data import save_zaragoza
    c = FO.SCATTERERS["16x16x64_r20"]
    rows, _, _, _, _ = FO.scatterer_scene(c)
    _, _, walls = FO.lattice(c["H"], c["W"], c["sx"], c["sz"])
    data = np.zeros((84, c["H"], c["W"]), dtype=np.float32)
    data[20:84] = rows.T.reshape(64, c["H"], c["W"])
    lg = {None: None, "one": np.array([[0.11], [0.0], [-0.07]], dtype=np.float32),
          "each": (walls + np.array([0.1, 0.0, 0.0], dtype=np.float32)[None]).T}[lasers]
    save_zaragoza(path, data, walls.T, (0.0, 0.7, 0.0), 0.61, c["dr"], 1.0, laser_grid_positions=lg)


def captures_and_command_lines():
    from nlosgr.data import make_data_kwargs
    wl = str(3 * 0.0625)
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)                                              # (the printed lines name the files as given)
        for lasers in (None, "one", "each"):
            cap = f"cap_{lasers}.mat"
            write_capture(cap, lasers)
            for shuffle in (False, True):
                torch.manual_seed(6)
                dk, *_ = make_data_kwargs(cap, DEV, shuffle=shuffle)
                for crop in (True, False):
                    tag = f"{lasers} shuffle{int(shuffle)} crop{int(crop)}"
                    emit(f"fk_capture {tag}", lambda: fk.fk_capture(dk, 20, 84, crop=crop))
                    emit(f"lct_capture {tag}", lambda: lct.lct_capture(dk, 20, 84, snr=2.0, nv=96, crop=crop))
                    emit(f"lct_solve_capture {tag}", lambda: lct.lct_solve_capture(dk, 20, 84, iterations=3, crop=crop))
                    emit(f"rsd_capture {tag}", lambda: rsd.rsd_capture(dk, 9, 20, 84, float(wl), crop=crop))
            window = [cap, "--start", "20", "--end", "84"]
            for mod, argv in ((backproject, ["--resolution", "16", "--power", "1"]),
                              (phasor, ["--resolution", "16", "--wavelength", wl]),
                              (forward_project, ["--resolution", "8", "--iterations", "3"]),
                              (fk, ["--no-amplitude"]), (fk, ["--mesh", "fk.ply", "--level-frac", "0.3"]),
                              (rsd, ["--resolution", "9", "--wavelength", wl, "--mesh", "rsd.ply"]),
                              (lct, ["--snr", "2", "--nv", "96"]), (lct, ["--backprop", "--power", "2"]),
                              (lct, ["--iterations", "3", "--no-accelerate", "--falloff", "2", "--mesh", "lct.ply"])):
                def run():
                    out = io.StringIO()
                    with contextlib.redirect_stdout(out):
                        mod.main(window + argv + ["--out", "out.npz"])
                    z = np.load("out.npz")
                    return {k: z[k] for k in z.files}, out.getvalue()
                emit(f"main {mod.__name__} {lasers} {' '.join(argv)}", run)
        os.chdir("/")


if __name__ == "__main__":
    if ARGS.host_only:
        host_only()
    else:
        assert torch.cuda.is_available(), "lattice_digests needs a GPU (or --host-only)"
        stages()
        dense()
        captures_and_command_lines()
    print("cases", COUNT)
