"""The non-confocal Gaussian renderer without a GPU: its float64 oracle (tests/render_nc_oracle.py) against the
confocal oracle and against the voxel projector's measure, the host-side validation of the three entry points, and
data.volume_geometry_nc."""
import ctypes
import math

import numpy as np
import pytest
import torch

import nonconfocal_oracle as NO
import render_nc_oracle as NCO
import volume_oracle as VO


@pytest.mark.parametrize("scene", ["cuda", "torch"])
def test_lasers_on_the_sensors_is_the_confocal_oracle(scene):
    """d = tau and q = 1 exactly, so the rows are volume_oracle.wall_hist's (measured: difference 0.0)."""
    model, geo, _ = VO.compact_scene("cuda") if scene == "cuda" else VO.parity_scene("torch", "noocl", 97)
    P = VO.params_of_model(model)
    for cutoff in (0.0, 5.7):
        want = VO.forward(P, geo, scene, "noocl", 1.0, cutoff)
        got = NCO.forward(P, geo, geo.wall, scene, cutoff)
        top = want.abs().amax(dim=1, keepdim=True)
        rel = float(((got - want).abs() / top).max())
        print(f"{scene} cutoff {cutoff}: max |nc - confocal| / rowmax = {rel:.3e}")
        assert float(top.min()) > 0 and rel <= 1e-12
    one = NCO.forward(P, geo.slice(1, 2), geo.wall[1:2], scene, 5.7)
    assert torch.equal(one[0], NCO.forward(P, geo, geo.wall, scene, 5.7)[1])


def test_displaced_lasers_change_the_rows_and_empty_the_bins_no_path_reaches():
    model, geo, _ = VO.compact_scene("cuda")
    P = VO.params_of_model(model)
    tab = VO.tables(geo)
    r0, dr = float(tab["r"][0]), float(tab["r"][1] - tab["r"][0])
    lasers = geo.wall.clone()
    lasers[:, 0] += 0.25
    lasers[0] = geo.wall[0] + torch.tensor([2.0 * (r0 + 10.5 * dr), 0.0, 0.0])
    got = NCO.forward(P, geo, lasers, "cuda", 0.0)
    conf = NCO.forward(P, geo, geo.wall, "cuda", 0.0)
    assert bool((got[0, :11] == 0).all()) and bool((got[0, 11:] > 0).all())
    assert float((got[1:] - conf[1:]).abs().max()) > 1e-2 * float(conf.max())
    # a [1, 3] laser is the repeated spot
    a = NCO.forward(P, geo, lasers[1:2], "cuda", 5.7)
    b = NCO.forward(P, geo, lasers[1:2].expand(geo.nwall, 3).contiguous(), "cuda", 5.7)
    assert torch.equal(a, b)


def test_the_measure_against_the_voxel_projector():
    """One isotropic Gaussian well inside the window.  sum_k of the oracle's row with hscale = dtheta dphi and att =
    1 / tau^2 is  sum_k sum_ij sin(theta) dtheta dphi pdf / (dl D): times dr the integral of pdf / (dl^2 ds^2) dV,
    which nonconfocal_oracle.forward64(power=-4) of the voxelized Gaussian sums as sum_x pdf / (dl^2 ds^2), times
    dV.  Both are rectangle rules on a Gaussian at a third of its standard deviation per step (errors far below
    1e-3); a wrong measure (q = 1, or dl / D dropped) is off by tens of percent."""
    sig = 0.05
    s = torch.tensor([0.0, 0.0, 0.0], dtype=torch.float64)
    laser = torch.tensor([-0.7, 0.0, 0.3], dtype=torch.float64)
    mu = torch.tensor([0.1, -0.6, 0.05], dtype=torch.float64)
    P = VO.Params64(VO.R.Params(mu[None].float(), torch.full((1, 3), math.log(sig)), torch.tensor([[1.0, 0, 0, 0]]),
                                torch.zeros(1, 1), torch.full((1, 1, 1), 0.5 / VO.R.C0), torch.zeros(1, 0, 1), 0))
    mu = P._mu.detach()[0]
    dist = float(mu.norm())
    thc, phc = math.acos(float(mu[2]) / dist), math.atan2(float(mu[1]), float(mu[0]))
    n, half = 61, 0.5
    th = torch.linspace(thc - half, thc + half, n, dtype=torch.float64)
    ph = torch.linspace(phc - half, phc + half, n, dtype=torch.float64)
    dth = float(th[1] - th[0])
    gc = 0.5 * (dist + float((mu - laser).norm()))
    dr = sig / 3
    r = gc + dr * (torch.arange(61, dtype=torch.float64) - 30)
    tab = dict(wall=s[None], st=torch.sin(th)[None], ct=torch.cos(th)[None], sp=torch.sin(ph)[None],
               cp=torch.cos(ph)[None], r=r, att=1.0 / (r * r), hscale=torch.tensor([dth * dth], dtype=torch.float64))
    with torch.no_grad():
        row = NCO.hist_nc(P, tab, 0, laser, "cuda", None) / 0.5          # sigma = 1/2, rho = 1
        rays = float(row.sum())
        # the voxelized Gaussian through the projector
        m = 37
        tabs = [np.linspace(float(mu[c]) - 6 * sig, float(mu[c]) + 6 * sig, m) for c in range(3)]
        X = torch.from_numpy(np.stack(np.meshgrid(*tabs, indexing="ij"), axis=-1).reshape(-1, 3))
        vol = VO.R.gaussian_pdf(X, P, "cuda", 1.0, None)[0].numpy().reshape(m, m, m)
    dv = float(np.prod([t[1] - t[0] for t in tabs]))
    rows, _ = NO.forward64(vol, s[None].numpy(), laser[None].numpy(), *tabs, float(r[0]), 1.0 / dr, 61, -4, dmin=1e-3,
                           want_bound=False)
    vox = float(rows.sum()) * dv / dr
    print(f"rays {rays:.9e}  voxels {vox:.9e}  relative difference {abs(rays - vox) / vox:.2e}")
    assert abs(rays - vox) <= 1e-3 * vox
    with torch.no_grad():
        x, w, q = NCO.points_nc(tab, 0, laser)
        pdf = VO.R.gaussian_pdf(x.reshape(-1, 3), P, "cuda", 1.0, None).view(61, -1)
        confocal_measure = float((tab["hscale"][0] * tab["att"][:, None] * w[None] * pdf).sum())
    assert abs(confocal_measure - vox) > 0.05 * vox                       # q matters here


def _structs(_lib, fake, **kw):
    g = dict(ng=8, k_feat=16, sh_degree=3, preset=_lib.PRESET_CUDA, mod=1.0, ptr=fake)
    geo = dict(nwall=4, nt=6, np=6, nr=32, ptr=fake)
    o = dict(mode=0, cutoff=3.0, c_deltaT=1.0, ray_scale=1.0, nsplit=0, flags=0, ray_cache=0, selection=0, g_begin=0,
             g_end=0)
    for k, v in kw.items():
        (g if k in g else geo if k in geo else o)[k] = v
    G = _lib.Gaussians(g["ng"], g["k_feat"], g["sh_degree"], g["preset"], g["mod"], *([g["ptr"]] * 5))
    GEO = _lib.Geometry(geo["nwall"], geo["nt"], geo["np"], geo["nr"], *([geo["ptr"]] * 9))
    O = _lib.Options(o["mode"], o["cutoff"], o["c_deltaT"], o["ray_scale"], o["nsplit"], o["flags"], o["ray_cache"],
                     o["selection"], o["g_begin"], o["g_end"])
    return G, GEO, O


def test_entry_points_validate_on_the_host():
    """Every rejected input of the three entry points, with its code and message, before any launch (no GPU; the
    fake non-null pointers are never read)."""
    from nlosgr import _lib
    lib = _lib.load()
    for name in ("nlosgr_render_nc_workspace_bytes", "nlosgr_render_nc_fwd", "nlosgr_render_nc_bwd"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    fake = ctypes.c_void_p(4096)
    err = lib.nlosgr_last_error

    def calls(lasers=fake, nlaser=4, ws=fake, hist=fake, grad=fake, outs=fake, **kw):
        G, GEO, O = _structs(_lib, fake, **kw)
        size = lib.nlosgr_render_nc_workspace_bytes(G, GEO, nlaser, O)
        e0 = err()
        f = lib.nlosgr_render_nc_fwd(G, GEO, lasers, nlaser, O, ws, hist, None)
        e1 = err()
        b = lib.nlosgr_render_nc_bwd(G, GEO, lasers, nlaser, O, ws, grad, outs, outs, outs, outs, outs, None)
        return size, e0, f, e1, b, err()

    def rejected(code, word, **kw):
        size, e0, f, e1, b, e2 = calls(**kw)
        assert size == 0 and f == code and b == code, (kw, size, f, b)
        assert word in e0 and word in e1 and word in e2, (kw, e0, e1, e2)

    G, GEO, O = _structs(_lib, fake)
    assert lib.nlosgr_render_nc_workspace_bytes(G, GEO, 4, O) > 0
    assert lib.nlosgr_render_nc_workspace_bytes(G, GEO, 1, O) > 0
    # scope: NLOSGR_E_UNSUPPORTED
    for mode in (_lib.MODE_NETF, _lib.MODE_BININT, _lib.MODE_OCCL):
        rejected(3, b"NLOSGR_MODE_NOOCL", mode=mode)
    rejected(3, b"NLOSGR_SELECT_SUPPORT", selection=_lib.SELECT_AABB)
    rejected(3, b"ray_cache", ray_cache=1)
    # options that belong to the confocal renderer: NLOSGR_E_INVALID
    for kw in (dict(nsplit=2), dict(g_begin=256), dict(g_end=8), dict(flags=_lib.FLAG_FLOAT_DRAIN), dict(flags=1)):
        rejected(1, b"nsplit, g_begin, g_end and flags", **kw)
    # the lasers
    for nl in (0, 2, 3, 5, -1):
        rejected(1, b"nlaser", nlaser=nl)
    size, _, f, e1, b, e2 = calls(lasers=None)
    assert size > 0 and f == 1 and b == 1 and b"lasers" in e1 and b"lasers" in e2
    size, _, f, e1, b, e2 = calls(lasers=None, nlaser=1)
    assert f == 1 and b == 1 and b"lasers" in e1 and b"lasers" in e2
    # what nlosgr_render_fwd validates
    rejected(1, b"ng", ng=-1)
    rejected(1, b"preset", preset=7)
    rejected(3, b"active_sh_degree", sh_degree=4)                         # cuda preset stops at 3
    rejected(3, b"active_sh_degree", sh_degree=5, preset=_lib.PRESET_TORCH, k_feat=25)
    rejected(1, b"k_feat", k_feat=9)
    rejected(1, b"k_feat", k_feat=17)
    rejected(1, b"geometry sizes", nr=0)
    rejected(1, b"geometry sizes", nwall=-1, nlaser=1)
    rejected(3, b"nr <= 4096", nr=4097)
    rejected(3, b"nt, np <= 1024", nt=1025)
    size, _, f, e1, b, e2 = calls(ptr=None)                               # (one ptr for both structs' tables)
    assert size == 0 and f == 1 and b == 1 and b"null" in e1
    # null outputs, workspace
    size, _, f, e1, b, e2 = calls(hist=None)
    assert f == 1 and b"hist_out" in e1
    size, _, f, e1, b, e2 = calls(outs=None)
    assert b == 1 and b"gradient output" in e2
    size, _, f, e1, b, e2 = calls(ws=None)
    assert f == 1 and b == 1 and b"workspace" in e1 and b"workspace" in e2
    assert lib.nlosgr_render_nc_fwd(None, None, fake, 1, None, fake, fake, None) == 1 and b"null" in err()
    # valid without a launch: no measurements (forward), no Gaussians (backward), degree 4 in the torch preset
    G, GEO, O = _structs(_lib, fake, nwall=0)
    assert lib.nlosgr_render_nc_fwd(G, GEO, fake, 1, O, fake, fake, None) == 0
    G, GEO, O = _structs(_lib, fake, ng=0)
    assert lib.nlosgr_render_nc_bwd(G, GEO, fake, 4, O, None, fake, None, None, None, None, None, None) == 0
    G, GEO, O = _structs(_lib, fake, preset=_lib.PRESET_TORCH, sh_degree=4, k_feat=25)
    assert lib.nlosgr_render_nc_workspace_bytes(G, GEO, 4, O) > 0
    assert lib.nlosgr_abi_version() == 13


def _capture(tmp_path, lasers, name, H=3, W=4, T=6):
    from nlosgr.data import save_zaragoza
    g = np.random.default_rng(5)
    data = g.random((T, H, W)).astype(np.float32)
    sensors = g.random((3, H * W)).astype(np.float32)
    sensors[1] = 0.0
    path = str(tmp_path / name)
    save_zaragoza(path, data, sensors, (0.0, 0.5, 0.0), 0.5, 0.01, 1.0, laser_grid_positions=lasers)
    return path, sensors


def test_volume_geometry_nc(tmp_path):
    """The sensed points' tables in the shuffled column order with each column's own laser; a confocal file gives
    lasers == sensors; volume_geometry keeps refusing the non-confocal file and agrees on the confocal one."""
    from nlosgr.data import make_data_kwargs, volume_geometry, volume_geometry_nc
    g = np.random.default_rng(9)
    per = g.random((3, 12)).astype(np.float32)
    path, sensors = _capture(tmp_path, per, "nc.mat")
    torch.manual_seed(3)
    dk, _, pos, index = make_data_kwargs(path, "cpu", shuffle=True)
    idx = index.long().numpy()
    assert idx.tolist() != list(range(12))
    geo, lasers = volume_geometry_nc(dk, 4, 1, 5)
    assert geo.nwall == 12 and geo.nr == 4 and geo.nt == 4
    assert np.array_equal(geo.wall.numpy(), sensors[:, idx].T) and np.array_equal(lasers.numpy(), per[:, idx].T)
    assert lasers.dtype == torch.float32 and lasers.is_contiguous()
    with pytest.raises(NotImplementedError, match="confocal only"):
        volume_geometry(dk, 4, 1, 5)
    one, _ = _capture(tmp_path, per[:, :1].copy(), "one.mat")
    dk1, *_ = make_data_kwargs(one, "cpu", shuffle=True)
    geo1, lasers1 = volume_geometry_nc(dk1, 4, 1, 5)
    assert tuple(lasers1.shape) == (1, 3) and np.array_equal(lasers1.numpy(), per[:, :1].T)
    plain, _ = _capture(tmp_path, None, "plain.mat")
    torch.manual_seed(3)
    dk0, *_ = make_data_kwargs(plain, "cpu", shuffle=True)
    geo0, lasers0 = volume_geometry_nc(dk0, 4, 1, 5)
    ref = volume_geometry(dk0, 4, 1, 5)
    assert torch.equal(lasers0, geo0.wall) and lasers0.data_ptr() != geo0.wall.data_ptr()
    for name in ("wall", "sin_theta", "cos_theta", "sin_phi", "cos_phi", "grid_lin", "hscale", "r", "att"):
        assert torch.equal(getattr(geo0, name), getattr(ref, name)), name
        assert torch.equal(getattr(geo0, name), getattr(geo, name)), name   # the tables do not depend on the lasers


def test_python_surface_refuses_what_the_kernels_do_not_serve():
    from nlosgr.render import RenderConfig
    from nlosgr.render_nc import lasers_for, render_nc_forward
    model, geo, _ = VO.compact_scene("cuda")
    with pytest.raises(RuntimeError):                                     # CPU tensors: no fallback
        render_nc_forward(model._mu, model._scaling, model._rotation, model._opacity, torch.zeros(48, 16), geo,
                          geo.wall, RenderConfig(preset="cuda", sh_degree=3))
    with pytest.raises(RuntimeError):
        lasers_for(torch.zeros(3, 6), geo)                                # (the file's [3, n] layout, on the CPU)
