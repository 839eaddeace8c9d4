"""GPU tests of the voxelizer's backward (nlosgr.voxelize.voxelize_backward -> nlosgr_voxelize_bwd), its autograd
fronts (voxelize_params, forward_project.project) and its contract, against the float64 gradient oracle
(tests/voxel_grad_oracle.py) on the 150-Gaussian / 40x9x33 problem of tests/voxel_oracle.py plus one Gaussian whose
albedo clamp is active (0.5 + SH < 0).

Parity criterion, per Gaussian and per gradient tensor: e_g <= TOL s_g (voxel_grad_oracle: s_g is the row's largest
component under the positive plus under the negative part of the upstream; d_rotation carries the oracle's own
noise floor).  The upstream is seeded normal noise, zero on the voxels the oracle marks `near` a support boundary
(band 1e-4), so pairs on the discontinuous mask contribute nothing on either side.

TOL: the worst ratios max_g e_g / s_g measured on gfx950 (MI355X), the largest over the three upstream choices (G_d
only, G_a only, both):

    preset cutoff   mu       scaling  rotation opacity  features
    torch  0        1.9e-07  5.9e-08  2.5e-07  7.0e-08  7.3e-09
    torch  3        1.9e-07  5.9e-08  2.5e-07  7.0e-08  7.3e-09      (every std >= 1: nothing is cut, the three
    torch  5.7      1.9e-07  5.9e-08  2.5e-07  7.0e-08  7.3e-09       cutoffs evaluate the same pairs)
    cuda   0        7.3e-06  3.3e-06  7.3e-06  2.7e-06  1.4e-06
    cuda   3        7.3e-06  3.5e-06  7.3e-06  3.2e-06  1.3e-06
    cuda   5.7      7.5e-06  3.3e-06  7.3e-06  2.6e-06  1.5e-06

TOL = 4 x 7.5e-6 = 3.0e-5, rounded up to one significant digit: 4e-5.  The cuda preset's Gaussians span 2 to 6 voxels,
so their exponents d^T n d reach -6.5 (cutoff 3) from entries of n near 5e4; a few fp32 roundings of such an exponent
are a relative error of about 1e-6 in p, which the worst rows (Gaussians 95 and 113, a dozen voxels each) do not
average out.  The torch preset's wide Gaussians keep the exponent near 0 and sum thousands of voxels.
The workgroup path (test_wide_boxes_take_the_workgroup_path, 65x64x64 voxels) measured 2.5e-6 at worst (d_rotation of
the 0.01-std Gaussian); its two grid-sized Gaussians stay below 2e-8.
"""
import numpy as np
import pytest
import torch

import voxel_grad_oracle as GO
import voxel_oracle as VO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 4e-5
NG = 151
OUTSIDE = 146       # the hand-placed Gaussian whose support lies wholly outside the grid
CLAMPED = 150       # the appended Gaussian with 0.5 + SH < 0


def _model(p, deg=3, dev=DEV):
    from nlosgr import GaussianParams
    t = lambda k: torch.as_tensor(p[k]).float().to(dev).contiguous()
    return GaussianParams(t("mu"), t("scaling"), t("rotation"), t("opacity"), t("features_dc"), t("features_rest"),
                          deg, deg)


def _cam(c=VO.PARITY_CAM):
    return torch.tensor(c, dtype=torch.float32, device=DEV)


def gaussians(preset):
    """voxel_oracle.parity_gaussians plus one Gaussian inside the grid whose dc coefficient puts 0.5 + SH below 0."""
    p = VO.parity_gaussians(preset)
    std = 0.02
    extra = dict(mu=torch.tensor([[0.05, 0.49, -0.03]]), scaling=torch.log(torch.tensor([[std, 1.3 * std, 0.8 * std]])),
                 rotation=torch.tensor([[0.9, 0.1, -0.3, 0.2]]), opacity=torch.tensor([[0.4]]),
                 features_dc=torch.full((1, 1, 1), -3.0), features_rest=torch.zeros(1, 15, 1))
    return {k: torch.cat((v, extra[k]), dim=0) for k, v in p.items()}


@pytest.fixture(scope="module")
def prob():
    """Models on the GPU, float64 oracle parameters, the seeded upstream pair, and per (preset, cutoff) the `near`
    voxels and the oracle's support mask; references are computed on demand and cached."""
    from nlosgr.voxelize import VoxelGrid
    grid = VoxelGrid(axes=VO.parity_axes())
    coords = grid.coords()
    g = torch.Generator().manual_seed(17)
    out = {"grid": grid, "coords": coords, "gd": torch.randn(grid.shape, generator=g),
           "ga": torch.randn(grid.shape, generator=g), "ref": {}}
    for preset in ("torch", "cuda"):
        p = gaussians(preset)
        P = GO.params64(p, 3)
        out[preset] = {"p": p, "model": _model(p), "P": P}
        assert GO.R.albedo(P, torch.tensor(VO.PARITY_CAM).double(), preset)[CLAMPED].item() == 0.0
        for mc in (0.0, 3.0, 5.7):
            with torch.no_grad():
                _, _, near = VO.volumes(P, coords, VO.PARITY_CAM, preset, 1.0, mc if mc > 0 else None)
            out[preset][mc] = near
    return out


def _upstream(prob, preset, cutoff, which):
    keep = (~prob[preset][cutoff]).float()
    gd = prob["gd"] * keep if which in ("d", "both") else None
    ga = prob["ga"] * keep if which in ("a", "both") else None
    return gd, ga


def _reference(prob, preset, cutoff, which):
    key = (preset, cutoff, which)
    if key not in prob["ref"]:
        gd, ga = _upstream(prob, preset, cutoff, which)
        prob["ref"][key] = GO.reference(prob[preset]["P"], prob["coords"], VO.PARITY_CAM, preset, gd, ga,
                                        mc=cutoff if cutoff > 0 else None)
    return prob["ref"][key]


def _run(model, grid, gd, ga, preset, cutoff):
    from nlosgr.voxelize import voxelize_backward
    up = lambda t: None if t is None else t.to(DEV)
    return voxelize_backward(model, grid, _cam(), up(gd), up(ga), preset=preset, cutoff=cutoff)


def _equal(a, b):
    """bitwise equality of two tuples of tensors (NaN patterns included)"""
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("which", ["d", "a", "both"])
@pytest.mark.parametrize("cutoff", [0.0, 3.0, 5.7])
@pytest.mark.parametrize("preset", ["torch", "cuda"])
def test_parity_per_gaussian(prob, preset, cutoff, which):
    near = prob[preset][cutoff]
    share = near.float().mean().item()
    print(f"{preset} cutoff {cutoff}: excluded share {100 * share:.4f} %")
    assert share <= 0.005
    gd, ga = _upstream(prob, preset, cutoff, which)
    grads, scale = _reference(prob, preset, cutoff, which)
    got5 = _run(prob[preset]["model"], prob["grid"], gd, ga, preset, cutoff)
    got = GO.as_named(got5)
    r = GO.ratios(got, grads, scale, near.numel())
    for n in GO.NAMES:
        g = int(torch.argmax(r[n]))
        print(f"worst ratio {n:9s} {preset:5s} cutoff {cutoff} upstream {which:4s}: {r[n][g].item():.3e} (Gaussian {g}, "
              f"s_g {scale[n][g].item():.3e})")
    for n in GO.NAMES:
        bad = torch.nonzero(r[n] > TOL).reshape(-1).tolist()
        assert not bad, (n, [(g, r[n][g].item(), scale[n][g].item()) for g in bad[:8]])
    if cutoff > 0 and preset == "cuda":
        assert all((t[OUTSIDE] == 0).all() for t in got5)                    # wholly outside: exactly zero rows
    assert (got5[4][CLAMPED] == 0).all()                                       # the clamp stops dL/dfeatures
    assert which == "d" or got["features"][:145].abs().max() > 0


def test_two_runs_and_permutations_are_bitwise(prob):
    """Two runs are bitwise equal; a random permutation of the Gaussians permutes all five outputs bitwise, at
    cutoff 3 and in dense mode: a row depends on its own Gaussian alone."""
    grid, p = prob["grid"], prob["cuda"]["p"]
    perm = torch.randperm(NG, generator=torch.Generator().manual_seed(3))
    for cutoff in (3.0, 0.0):
        gd, ga = _upstream(prob, "cuda", cutoff, "both")
        a = _run(prob["cuda"]["model"], grid, gd, ga, "cuda", cutoff)
        b = _run(prob["cuda"]["model"], grid, gd, ga, "cuda", cutoff)
        assert _equal(a, b)
        c = _run(_model({k: v[perm] for k, v in p.items()}), grid, gd, ga, "cuda", cutoff)
        assert _equal(c, [t[perm.to(DEV)] for t in a]), cutoff
        assert a[0].abs().max() > 0


def test_appending_gaussians_leaves_the_rows_unchanged(prob):
    """100 more Gaussians after the 151: the first 151 rows are bitwise unchanged (no dependence on ng or on the
    launch shape: 38 workgroups become 63)."""
    from nlosgr import GaussianParams
    grid, p = prob["grid"], prob["cuda"]["p"]
    m = GaussianParams.synthetic(100, 3, preset="cuda", seed=9, volume_position=(0.0, 0.5, 0.0), volume_size=0.4)
    more = dict(mu=m._mu, scaling=m._scaling, rotation=m._rotation, opacity=m._opacity, features_dc=m._features_dc,
                features_rest=m._features_rest)
    q = {k: torch.cat((v, more[k].detach().cpu()), dim=0) for k, v in p.items()}
    gd, ga = _upstream(prob, "cuda", 3.0, "both")
    a = _run(prob["cuda"]["model"], grid, gd, ga, "cuda", 3.0)
    b = _run(_model(q), grid, gd, ga, "cuda", 3.0)
    assert b[0].shape[0] == NG + 100 and _equal([t[:NG] for t in b], a)
    assert b[0][NG:].abs().max() > 0


@pytest.mark.parametrize("cutoff", [0.0, 3.0])
def test_one_gaussian_and_one_voxel(prob, cutoff):
    """ng = 1 on the parity grid, and the whole problem on a 1x1x1 grid, against the oracle."""
    from nlosgr.voxelize import VoxelGrid
    p = {k: v[10:11] for k, v in prob["cuda"]["p"].items()}
    gd, ga = _upstream(prob, "cuda", cutoff, "both")
    got = GO.as_named(_run(_model(p), prob["grid"], gd, ga, "cuda", cutoff))
    grads, scale = GO.reference(GO.params64(p, 3), prob["coords"], VO.PARITY_CAM, "cuda", gd, ga,
                                mc=cutoff if cutoff > 0 else None)
    full = GO.as_named(_run(prob["cuda"]["model"], prob["grid"], gd, ga, "cuda", cutoff))
    for n in GO.NAMES:
        assert GO.ratios(got, grads, scale, gd.numel())[n].max() <= TOL, n
        assert torch.equal(got[n][0], full[n][10]), n                  # and bitwise its row of the full problem
    one = VoxelGrid(axes=((0.0125, 0.0125, 1), (0.5, 0.5, 1), (0.0125, 0.0125, 1)))
    u = torch.tensor([[[1.5]]]), torch.tensor([[[-0.7]]])
    got = GO.as_named(_run(prob["cuda"]["model"], one, u[0], u[1], "cuda", cutoff))
    grads, scale = GO.reference(prob["cuda"]["P"], one.coords(), VO.PARITY_CAM, "cuda", u[0], u[1],
                                mc=cutoff if cutoff > 0 else None)
    m2 = -2.0 * torch.log(GO.R.gaussian_pdf(one.coords().reshape(-1, 3).double(), prob["cuda"]["P"], "cuda").detach())
    assert cutoff == 0 or ((m2 - cutoff ** 2).abs() > 1e-4 * cutoff ** 2).all()
    assert grads["mu"].abs().max() > 0
    for n in GO.NAMES:
        assert GO.ratios(got, grads, scale, 1)[n].max() <= TOL, n


def test_no_upstream_gives_zeros(prob):
    for cutoff in (0.0, 3.0):
        out = _run(prob["cuda"]["model"], prob["grid"], None, None, "cuda", cutoff)
        assert [tuple(t.shape) for t in out] == [(NG, 3), (NG, 3), (NG, 4), (NG,), (NG, 16)]
        assert all((t == 0).all() for t in out)


def test_nan_gaussian_gets_zero_rows(prob):
    """A Gaussian with a NaN mu inserted at index 75: at cutoff 3 its box is not finite, so its rows are zero, as the
    forward skips it, and every other row is bitwise unchanged."""
    p = prob["cuda"]["p"]
    q = {}
    for k, v in p.items():
        row = v[75:76].clone()
        if k == "mu":
            row[0, 1] = float("nan")
        q[k] = torch.cat((v[:75], row, v[75:]), dim=0)
    gd, ga = _upstream(prob, "cuda", 3.0, "both")
    want = _run(prob["cuda"]["model"], prob["grid"], gd, ga, "cuda", 3.0)
    got = _run(_model(q), prob["grid"], gd, ga, "cuda", 3.0)
    assert got[0].shape[0] == NG + 1
    assert all((t[75] == 0).all() for t in got)
    assert _equal([torch.cat((t[:75], t[76:])) for t in got], want)


def test_nan_upstream_reaches_exactly_the_supports_that_hold_it(prob):
    """A NaN in both upstreams at one voxel (not `near` any support boundary), cutoff 3: the rows that turn NaN are
    exactly those of the Gaussians whose support, by the oracle's mask, holds the voxel; the masked pairs are
    dropped by a select, so the NaN does not reach anyone else."""
    near = prob["cuda"][3.0].reshape(-1)
    mask = GO.support_mask(prob["cuda"]["P"], prob["coords"], "cuda", mc=3.0)       # [Ng, nvox]
    count = mask.sum(dim=0)
    count[near] = 0
    v = int(torch.argmax(count))
    hit = mask[:, v]
    assert 2 <= int(hit.sum()) < NG and not bool(hit[OUTSIDE])
    gd, ga = _upstream(prob, "cuda", 3.0, "both")
    gd, ga = gd.clone(), ga.clone()
    gd.view(-1)[v] = float("nan")
    ga.view(-1)[v] = float("nan")
    clean = _run(prob["cuda"]["model"], prob["grid"], *_upstream(prob, "cuda", 3.0, "both"), "cuda", 3.0)
    got = _run(prob["cuda"]["model"], prob["grid"], gd, ga, "cuda", 3.0)
    for t, name in zip(got[:4], ("mu", "scaling", "rotation", "opacity")):
        isnan = torch.isnan(t.reshape(NG, -1)).any(dim=1).cpu()
        assert torch.equal(isnan, hit), (name, torch.nonzero(isnan != hit).reshape(-1).tolist())
    fnan = torch.isnan(got[4]).any(dim=1).cpu()
    assert not bool(fnan[~hit].any())
    assert _equal([t[(~hit).to(DEV)] for t in got], [t[(~hit).to(DEV)] for t in clean])


def test_autograd_front_of_the_voxelizer(prob):
    """voxelize_params: the outputs are voxelize's bitwise, .backward() leaves .grad bitwise voxelize_backward's, and
    an output that is not wanted is None and costs no upstream."""
    from nlosgr.model import features_flat
    from nlosgr.voxelize import voxelize, voxelize_backward, voxelize_params
    m, grid = prob["cuda"]["model"], prob["grid"]
    leaves = [t.detach().clone().requires_grad_(True) for t in (m._mu, m._scaling, m._rotation, m._opacity,
                                                                features_flat(m))]
    dens, alb = voxelize_params(*leaves, grid, _cam(), preset="cuda", cutoff=3.0, sh_degree=3)
    wd, wa = voxelize(m, grid, _cam(), preset="cuda", cutoff=3.0)
    assert torch.equal(dens, wd) and torch.equal(alb, wa)
    gd, ga = [t.to(DEV) for t in _upstream(prob, "cuda", 3.0, "both")]
    ((dens * gd).sum() + (alb * ga).sum()).backward()
    want = voxelize_backward(m, grid, _cam(), gd, ga, preset="cuda", cutoff=3.0)
    got = [leaves[0].grad, leaves[1].grad, leaves[2].grad, leaves[3].grad.reshape(-1), leaves[4].grad]
    assert leaves[3].grad.shape == m._opacity.shape and _equal(got, want)
    for t in leaves:
        t.grad = None
    none_d, alb2 = voxelize_params(*leaves, grid, _cam(), preset="cuda", cutoff=3.0, sh_degree=3, want_density=False)
    assert none_d is None and torch.equal(alb2, wa)
    (alb2 * ga).sum().backward()
    want = voxelize_backward(m, grid, _cam(), None, ga, preset="cuda", cutoff=3.0)
    assert _equal([leaves[0].grad, leaves[1].grad, leaves[2].grad, leaves[3].grad.reshape(-1), leaves[4].grad], want)


@pytest.mark.parametrize("lasers", [False, True])
def test_autograd_front_of_the_projector(lasers):
    """forward_project.project: the rows are forward_project's bitwise, the volume's .grad is bitwise backproject of
    the upstream rows, and a negative power on a volume that requires grad raises."""
    from nlosgr.backproject import backproject
    from nlosgr.forward_project import forward_project, project
    from nlosgr.voxelize import VoxelGrid
    g = torch.Generator().manual_seed(4)
    grid = VoxelGrid((0.0, 0.5, 0.0), 0.5, 16)
    u = torch.linspace(-0.4, 0.4, 6)
    walls = torch.stack(torch.meshgrid(u, torch.zeros(1), u, indexing="ij"), -1).reshape(-1, 3).to(DEV).contiguous()
    ls = torch.tensor([[0.1, 0.0, -0.2]], device=DEV) if lasers else None
    vol = torch.rand(16, 16, 16, generator=g).to(DEV).requires_grad_(True)
    up = torch.randn(36, 64, generator=g).to(DEV)
    rows = project(vol, walls, grid, 0.2, 0.0125, 64, power=2, lasers=ls)
    assert torch.equal(rows, forward_project(vol.detach(), walls, grid, 0.2, 0.0125, 64, power=2, lasers=ls))
    (rows * up).sum().backward()
    assert torch.equal(vol.grad, backproject(up, walls, grid, 0.2, 0.0125, power=2, lasers=ls))
    assert vol.grad.abs().max() > 0
    with pytest.raises(ValueError, match="backproject"):
        project(vol, walls, grid, 0.2, 0.0125, 64, power=-4, lasers=ls)
    if not lasers:       # without grad the negative powers of forward_project stay available
        out = project(vol.detach(), walls, grid, 0.2, 0.0125, 64, power=-4)
        assert torch.equal(out, forward_project(vol.detach(), walls, grid, 0.2, 0.0125, 64, power=-4))


@pytest.mark.parametrize("cutoff", [0.0, 3.0])
def test_wide_boxes_take_the_workgroup_path(cutoff):
    """A 65x64x64 grid (266,240 voxels, just above the 2^18 a single wave walks) with six Gaussians of std 0.5 and 0.2
    (their cutoff-3 boxes are the whole grid: the workgroup path), 0.05, 0.03, 0.01 and 0.004 (the wave path); in
    dense mode every box is the grid.  Per-Gaussian parity against the oracle, and the rows of the reversed
    order are the reversed rows bitwise: which kernel sums a Gaussian depends on its box alone."""
    from nlosgr.voxelize import VoxelGrid
    g = torch.Generator().manual_seed(23)
    n, K = 6, 16
    std = torch.tensor([0.5, 0.2, 0.05, 0.03, 0.01, 0.004]).reshape(n, 1)
    p = dict(mu=(torch.rand(n, 3, generator=g) - 0.5) * 0.3 + torch.tensor([0.0, 0.5, 0.0]),
             scaling=torch.log(std) + 0.15 * torch.randn(n, 3, generator=g), rotation=torch.randn(n, 4, generator=g),
             opacity=torch.randn(n, 1, generator=g),
             features_dc=((0.1 + 0.3 * torch.rand(n, 1, 1, generator=g)) - 0.5) / GO.R.C0,
             features_rest=0.05 * torch.randn(n, K - 1, 1, generator=g))
    h = 0.5 / 64
    grid = VoxelGrid(axes=((-0.25, -0.25 + 64 * h, 65), (0.25, 0.25 + 63 * h, 64), (-0.25, -0.25 + 63 * h, 64)))
    assert grid.shape[0] * grid.shape[1] * grid.shape[2] > 2 ** 18
    coords = grid.coords()
    P = GO.params64(p, 3)
    mc = cutoff if cutoff > 0 else None
    with torch.no_grad():
        _, _, near = VO.volumes(P, coords, VO.PARITY_CAM, "cuda", 1.0, mc)
    assert near.float().mean().item() <= 0.005
    keep = (~near).float()
    gd, ga = torch.randn(grid.shape, generator=g) * keep, torch.randn(grid.shape, generator=g) * keep
    grads, scale = GO.reference(P, coords, VO.PARITY_CAM, "cuda", gd, ga, mc=mc)
    got5 = _run(_model(p), grid, gd, ga, "cuda", cutoff)
    r = GO.ratios(GO.as_named(got5), grads, scale, near.numel())
    for nme in GO.NAMES:
        print(f"worst ratio {nme:9s} wide, cutoff {cutoff}: " + " ".join(f"{v:.2e}" for v in r[nme].tolist()))
    for nme in GO.NAMES:
        assert grads[nme].abs().amax(dim=1).min() > 0 and r[nme].max() <= TOL, (nme, r[nme].tolist())
    rev = torch.arange(n - 1, -1, -1)
    back = _run(_model({k: v[rev] for k, v in p.items()}), grid, gd, ga, "cuda", cutoff)
    assert _equal(back, [t[rev.to(DEV)] for t in got5])
    assert _equal(_run(_model(p), grid, gd, ga, "cuda", cutoff), got5)
