"""CPU checks of tests/rays_oracle.py: the float64 reference against oracle.torch_ref.render_rays_cuda and a literal
march, the metric's scale, and what tests/test_gpu_rays_edges.py relies on in its scenes without a GPU: the
occlusion decision margins, the selected counts, the first-dead positions, the filter cases, and the tolerances
(8 x the fp32 oracle's worst value over scenes A, B and D)."""
import math

import pytest
import torch

from conftest import ROOT  # noqa: F401

import rays_oracle as RO
import volume_oracle as VO

PRESETS = ("cuda", "torch")


def test_reference_is_render_rays_cuda_in_float64():
    """cuda preset: reference() and oracle.torch_ref.render_rays_cuda on Params64 leaves are the same numbers,
    forward and gradients (1 - exp(-x) against expm1 differ by 1e-16 absolute in double)."""
    from oracle import torch_ref as R
    for occl in (False, True):
        sc = RO.scene_D("cuda", occl)
        ups = sc.upstreams()
        ref = sc.reference(ups)
        P = VO.Params64(sc.P)
        outs = R.render_rays_cuda(sc.o.double(), sc.d.double(), sc.t.double(), P, P.features[:, :, 0], sc.cam.double(),
                                  sc.deg, 1.0, sc.cdt, 1.0, occl, sc.filt)
        assert all(x.dtype == torch.float64 for x in outs)
        for a, b in zip(outs, ref.fwd):
            assert float((a.detach() - b).abs().max()) <= 1e-13 * max(float(b.abs().max()), 1.0)
        sum((a * u.double()).sum() for a, u in zip(outs, ups)).backward()
        for n, leaf in zip(VO.NAMES, P.leaves()):
            g = leaf.grad.reshape(ref.grads[n].shape)
            assert g.numel() == 0 or float((g - ref.grads[n]).abs().max()) <= 1e-10 * float(ref.scale[n].max())


@pytest.mark.parametrize("preset", PRESETS)
def test_reference_matches_a_literal_march(preset):
    """Both presets: a per-ray, per-sample loop over the row's Gaussians with the running transmittance and the
    early exit gives the reference's three outputs."""
    from oracle import torch_ref as R
    sc = RO.scene_A(65, preset, True)
    ref = sc.reference()
    P = VO.Params64(sc.P)
    with torch.no_grad():
        o, d, t, cam = sc.o.double(), sc.d.double(), sc.t.double(), sc.cam.double()
        x = (o[:, None, :] + d[:, None, :] * t[None, :, None]).reshape(-1, 3)
        pdf = R.gaussian_pdf(x, P, preset).view(-1, o.shape[0], t.shape[0])
        sig = torch.sigmoid(P._opacity)[:, 0]
        rho_g = R.albedo(P, cam, preset)[:, 0]
        exits = 0
        for r in range(o.shape[0]):
            idx = sc.filt[r, 1:1 + int(sc.filt[r, 0])].long()
            T = 1.0
            for s in range(t.shape[0]):
                c = pdf[idx, r, s] * sig[idx]
                if T < RO.T_DEAD:
                    assert float(ref.rho[r, s]) == 0.0 and float(ref.density[r, s]) == 0.0 and float(ref.trans[r, s]) == 0.0
                    exits += s == ref.first_dead()[r]
                else:
                    W = float(((1.0 - torch.exp(-c * sc.cdt)) * rho_g[idx]).sum())
                    assert math.isclose(float(ref.trans[r, s]), T, rel_tol=1e-12)
                    assert math.isclose(float(ref.rho[r, s]), T * W, rel_tol=1e-9, abs_tol=1e-15)
                    assert math.isclose(float(ref.density[r, s]), float(c.sum()), rel_tol=1e-12)
                T = T * math.exp(-float(c.sum()) * sc.cdt)
        assert exits >= 1


def test_scale_bounds_the_gradient_and_splits_by_sign():
    sc = RO.scene_D("cuda", True)
    ups = sc.upstreams()
    ref = sc.reference(ups)
    for n in VO.NAMES:
        assert bool((VO._rowmax(ref.grads[n]) <= ref.scale[n] * (1 + 1e-12)).all())
    assert float(ref.scale["opacity"].min()) > 0
    # a one-signed single upstream has one part: s_g is the row maximum of the gradient itself
    one = sc.reference((ups[0].abs(), None, None))
    for n in VO.NAMES:
        assert torch.allclose(VO._rowmax(one.grads[n]), one.scale[n], rtol=1e-12, atol=0)
    # the gradient is linear in the upstream: the parts add up
    both = sc.reference((ups[0], ups[1], None))
    a, b = sc.reference((ups[0], None, None)), sc.reference((None, ups[1], None))
    for n in VO.NAMES:
        assert torch.allclose(both.grads[n], a.grads[n] + b.grads[n], rtol=1e-10, atol=1e-14)
        assert torch.all(both.scale[n] <= (a.scale[n] + b.scale[n]) * (1 + 1e-12))


def _occlusion_scenes(preset):
    out = [(f"A{n}", RO.scene_A(n, preset, True)) for n in RO.A_NSAMP]
    out += [(f"B{c}", RO.scene_B(c, preset, True)) for c in RO.B_COUNTS]
    out += [("C", RO.scene_C(preset, True)), ("D", RO.scene_D(preset, True)), ("D16", RO.scene_D(preset, True, True)),
            ("E", RO.scene_E(preset, True))]
    return out


@pytest.mark.parametrize("preset", PRESETS)
def test_occlusion_scenes_keep_their_margin(preset):
    """Every occlusion scene of test_gpu_rays_edges.py stays 1e-3 away from T = 1e-4 on every sample, dead or alive,
    and its first dead samples are where the scene's description puts them."""
    dead_at = {}
    for name, sc in _occlusion_scenes(preset):
        ref = sc.reference()
        assert ref.margin >= RO.MARGIN, (name, ref.margin)
        assert bool((ref.dead[:, 1:] >= ref.dead[:, :-1]).all())     # once dead, dead
        dead_at[name] = ref.first_dead()
    for n in RO.A_NSAMP:
        want = RO.A_FIRST_DEAD[n]
        assert dead_at[f"A{n}"][0] == (-1 if want is None else want)
        assert dead_at[f"A{n}"][4] == -1                             # the one-Gaussian ray never dies
    assert dead_at["A64"][0] == 63 and dead_at["A65"][0] == 64       # lane 63 of chunk 0, lane 0 of chunk 1
    assert dead_at["A129"][0] == 128 and 128 < dead_at["A200"][0] < 192   # lane 0 of and inside chunk 2
    for c in RO.B_COUNTS:
        big = max(range(len(c)), key=lambda r: c[r])
        assert dead_at[f"B{c}"][big] == (40 if c[big] >= 64 else -1)
        assert all(dead_at[f"B{c}"][r] == -1 for r in range(len(c)) if c[r] <= 1)
    assert dead_at["C"][1024] == 40 and len(set(dead_at["C"])) >= 4 and dead_at["C"][:3] == [-1, -1, -1]
    assert dead_at["D"][0] == 100 and dead_at["D16"][0] == 100
    assert dead_at["E"] == [2000, -1]


def test_scene_rows_and_sizes():
    for c in RO.B_COUNTS:
        sc = RO.scene_B(c, "cuda", False)
        assert sc.filt[:, 0].tolist() == list(c) and sc.P._mu.shape[0] == 300
        for r, n in enumerate(c):
            row = sc.filt[r, 1:1 + n]
            assert bool((row[1:] > row[:-1]).all()) and bool((sc.filt[r, 1 + n:] == -1).all())
        unnamed = int((~RO.row_mask(sc.filt, 300).any(dim=1)).sum())
        assert unnamed >= max(300 - sum(c), 30) and (c != (256,) or unnamed == 44)
    sc = RO.scene_C("torch", False)
    n = sc.filt[:, 0]
    assert sc.o.shape[0] == 1030 and sc.t.shape[0] == 65 and 6 <= sc.P._mu.shape[0] <= 8
    assert n[:3].tolist() == [0, 0, 0] and n[1027:].tolist() == [0, 0, 0] and int((n == 0).sum()) == 6
    assert not torch.equal(sc.d[0], sc.d[1024]) and torch.equal(sc.d[0], sc.d[10])
    sc = RO.scene_D("cuda", False, k16=True)
    assert sc.feats.shape == (12, 16) and sc.deg == 1
    sc = RO.scene_E("cuda", True)
    assert sc.t.shape[0] == 8192 and sc.o.shape[0] == 2
    for ns in RO.A_NSAMP:
        t = RO.t_grid(ns)
        assert t.shape[0] == ns and t.dtype == torch.float32 and bool((t[1:] > t[:-1]).all())
    assert {RO.DEG[(p, o)] for p in PRESETS for o in (False, True)} == {0, 1, 2, 3}


def test_empty_row_and_no_occlusion_are_exact():
    sc = RO.scene_B((0, 1, 64), "cuda", True)
    ref = sc.reference(sc.upstreams())
    assert bool((ref.rho[0] == 0).all()) and bool((ref.density[0] == 0).all()) and bool((ref.trans[0] == 1).all())
    for n in VO.NAMES:
        assert bool((ref.grads[n][~ref.named] == 0).all()) and bool((ref.scale[n][~ref.named] == 0).all())
    free = RO.scene_B((0, 1, 64), "cuda", False).reference()
    assert bool((free.trans == 1).all()) and free.margin == float("inf") and not bool(free.dead.any())


def test_filter_cases():
    """The 256th hit inside a block with more hits behind it; the special rays select what their comments say."""
    from oracle import torch_ref as R
    o, d, bb, moved = RO.cap_midblock_boxes()
    ref = R.aabb_filter(o, d, bb)
    hits = torch.nonzero(~moved).flatten()
    last = int(hits[255])
    assert hits.numel() > 256 and last % 64 < 60
    assert int(((hits > last) & (hits // 64 == last // 64)).sum()) > 0
    assert ref[:, 0].tolist() == [256, 0, 256] and torch.equal(ref[0, 1:], hits[:256].int())
    assert RO.slab_margin(o, d, bb) > 1e-6
    o, d, bb, want = RO.special_rays()
    ref = R.aabb_filter(o, d, bb)
    for r, idx in enumerate(want):
        assert ref[r, :1 + len(idx)].tolist() == [len(idx)] + idx, r
    assert bool((d == 0).any(dim=1).sum() >= 4) and bool((d < 0).any())
    for ng in RO.F_NG:
        hits = 0
        for nrays in RO.F_NRAYS:
            oo, dd, bb = RO.filter_case(ng, nrays)
            assert RO.slab_margin(oo, dd, bb) > 1e-6
            n = int(R.aabb_filter(oo, dd, bb)[:, 0].sum())
            hits += n
            assert ng < 63 or 0 < n < ng * nrays        # some hit, some miss
        assert (hits > 0) == (ng > 0)


def test_tolerances_are_eight_times_the_fp32_oracle():
    """The fp32 oracle (the same sums in fp32, torch autograd) in the per-Gaussian metric over scenes A, B and D:
    its worst value times 8, rounded up to one digit, is TOL / FWD_TOL where those are not capped."""
    worst = {}
    for preset in PRESETS:
        for occl in (False, True):
            cases = [(RO.scene_A(n, preset, occl), None) for n in RO.A_NSAMP]
            cases += [(RO.scene_B(c, preset, occl), None) for c in RO.B_COUNTS]
            for k16 in (False, True):
                sc = RO.scene_D(preset, occl, k16)
                u = sc.upstreams()
                cases += [(sc, x) for x in ((u[0], None, None), (None, u[1], None), (None, None, u[2]), u)]
                cases += [(sc, RO.one_hot(sc, s)) for s in (0, 63, 64, RO.D_NSAMP - 1)]
            for sc, ups in cases:
                ups = sc.upstreams() if ups is None else ups
                ref = sc.reference(ups)
                outs, grads = sc.fp32(ups)
                for n, v in VO.worst(VO.as_named(grads), ref).items():
                    worst[n] = max(worst.get(n, 0.0), v)
                for n, v in RO.forward_worst(outs, ref).items():
                    worst[(occl, n)] = max(worst.get((occl, n), 0.0), v)
    # (the window: rounding 8 x worst up to one digit puts it in (TOL / 2, TOL]; a quarter more for the run-to-run
    # spread of an fp32 sum's order on another CPU)
    for n in VO.NAMES:
        assert 0.4 * RO.TOL[n] <= 8 * worst[n] <= 1.25 * RO.TOL[n], (n, worst[n])
    for occl in (False, True):
        for n in RO.OUTPUTS:
            v, tol, cap = worst[(occl, n)], RO.FWD_TOL[occl][n], (2e-4 if occl else 2e-5)
            if v == 0.0:
                assert tol == 0.0
            elif 8 * v > 1.25 * tol:
                assert tol == cap, (occl, n, v)              # capped at what test_gpu_rays.py promises
            else:
                assert 0.4 * tol <= 8 * v, (occl, n, v)
