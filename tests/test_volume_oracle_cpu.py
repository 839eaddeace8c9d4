"""Pins the float64 volume reference (tests/volume_oracle.py) and its per-Gaussian metric.  No GPU is touched.

The reference is compared with the fp32 oracle (oracle.torch_ref.render_volume, itself pinned to the reference
implementation's golden vectors by test_oracle_golden.py) on the scene of test_gpu_parity.py::_volume_vs_oracle:
the forward within FWD_TOL of every row's maximum, every gradient within GAUSS_TOL per Gaussian in the metric of
volume_oracle (e_g <= tol s_g + b_g).  Both bounds are a few times the fp32 oracle's own rounding (measured:
3e-7 forward; per Gaussian <= 1.4e-6 on the broad scenes).  The narrow scene (log-scales - 3.5: Gaussians a
fraction of a bin wide, whose few samples sit on the steep flank of the pdf, where the fp32 rounding of a
sample's position is amplified by m^2 / 2 ~ 16) has bounds of its own, ten times the general ones: NARROW_TOL per
Gaussian (measured there <= 2.1e-5) and NARROW_FWD_TOL for the forward (measured 5.0e-6, the same amplification).

The per-bin forward metric (volume_oracle.forward_bins / forward_bin_failures) is pinned in three ways, on the
scenes tests/test_gpu_fwd_edges.py runs and at their sizes: (a) the fp32 oracle passes it at 2e-5 with no rounding
allowance, so the tolerance is not below fp32 noise; (b) four synthetic faults of one ray of one Gaussian, planted
in the float64 reference, are rejected even at the coarsest fixed-point unit the scene allows, while the row-maximum
figure the earlier forward tests use lets the first two pass; (c) in at least three quarters of the non-empty bins
neither the dense-culled bracket nor the rounding bound is what decides.

The per-ray outputs, the per-ray upstream, occlusion compositing and AABB selection of the reference are pinned to
the fp32 oracle (oracle.torch_ref.render_rays_cuda / aabb_filter) and to autograd of single samples; and every scene
that tests/test_gpu_ray_upstream.py and tests/test_gpu_tile_edges.py judge against the reference is shown to stay 1e-3
away from the model's discontinuous decisions (volume_oracle.decision_margins): that is where their seeds are proven.
"""
import pytest
import torch

from conftest import ROOT  # noqa: F401

import volume_oracle as VO
from oracle import torch_ref as R

FWD_TOL = 5e-6
GAUSS_TOL = 1e-5
NARROW_TOL = 1e-4       # the narrow scene only (module docstring)
NARROW_FWD_TOL = 5e-5


def _fp32_oracle(model, k, preset, mode, cutoff, gout):
    P = VO.params_of_model(model)
    hist = R.render_volume(P, k["walls"], k["box"], k["Y"], k["ns"], k["start"], k["end"], k["c"], k["deltaT"],
                           preset=preset, mode=mode, mc=cutoff if cutoff > 0 else None)
    (hist * gout).sum().backward()
    return P, hist.detach(), [l.grad for l in P.leaves()]


def _compare(preset, mode, T, cutoff, tol, scale_shift=None, fwd_tol=FWD_TOL):
    model, geo, k = VO.parity_scene(preset, mode, T, scale_shift=scale_shift)
    gout = torch.randn(geo.nwall, geo.nr, generator=torch.Generator().manual_seed(5))
    P, hist, grads = _fp32_oracle(model, k, preset, mode, cutoff, gout)
    ref = VO.reference(P, geo, preset, mode, k["c"] * k["deltaT"], cutoff, gout)
    fw = VO.forward_worst(hist, ref)
    w = VO.worst(grads, ref)
    print(f"\n{preset} {mode} T={T} cutoff={cutoff} shift={scale_shift}: forward {fw:.2e}; per Gaussian "
          + ", ".join(f"{n} {v:.2e}" for n, v in w.items()))
    assert fw <= fwd_tol
    bad = VO.failures(grads, ref, tol)
    assert not bad, bad[:5]
    return ref


@pytest.mark.parametrize("preset", ["torch", "cuda"])
@pytest.mark.parametrize("mode", ["noocl", "netf"])
@pytest.mark.parametrize("T", [41, 97])
@pytest.mark.parametrize("cutoff", [5.7, 0.0])
def test_reference_matches_fp32_oracle(preset, mode, T, cutoff):
    """Odd row lengths, both presets and modes, 5.7 sigma and dense; on these broad Gaussians nothing is culled,
    so the bracket is exactly zero."""
    ref = _compare(preset, mode, T, cutoff, GAUSS_TOL)
    assert all(float(b.max()) == 0.0 for b in ref.bracket.values())
    assert all(float(s.min()) > 0.0 for s in ref.scale.values())


@pytest.mark.parametrize("mode", ["noocl", "netf"])
def test_reference_matches_fp32_oracle_narrow(mode):
    """The narrow scene under its own bound; its bracket is live and some Gaussians are reached by no sample."""
    ref = _compare("cuda", mode, 97, 5.7, NARROW_TOL, scale_shift=-3.5, fwd_tol=NARROW_FWD_TOL)
    s = ref.scale["mu"]
    assert int((s > 0).sum()) * 3 >= s.numel() and int((s == 0).sum()) > 0
    assert float(ref.bracket["mu"].max()) > 0.0


@pytest.mark.parametrize("name,g", [("mu", 7), ("opacity", 0), ("features_rest", 47)])
def test_planted_error_fails_exactly_that_gaussian(name, g):
    """1e-3 s_g added to one component of one Gaussian's row of one tensor fails that Gaussian of that tensor and
    nothing else at the tolerance of 2e-4; the reference's own gradients pass at zero tolerance; worst() reports
    the planted 1e-3."""
    model, geo, k = VO.parity_scene("cuda", "netf", 41)
    gout = torch.randn(geo.nwall, geo.nr, generator=torch.Generator().manual_seed(5))
    ref = VO.reference(VO.params_of_model(model), geo, "cuda", "netf", k["c"] * k["deltaT"], 5.7, gout)
    got = {n: t.clone() for n, t in ref.grads.items()}
    assert VO.failures(got, ref, 0.0) == []
    got[name][g, -1] += 1e-3 * ref.scale[name][g]
    bad = VO.failures(got, ref, 2e-4)
    assert [(b[0], b[1]) for b in bad] == [(name, g)], bad
    w = VO.worst(got, ref)
    assert abs(w[name] - 1e-3) < 1e-9 and all(v == 0.0 for n, v in w.items() if n != name)
    assert VO.failures(got, ref, 2e-3) == []


def test_unreached_gaussian_must_stay_within_bracket():
    """A Gaussian no sample reaches (s_g = 0) fails as soon as it is given a gradient beyond b_g."""
    model, geo, k = VO.parity_scene("cuda", "noocl", 97, scale_shift=-3.5)
    gout = torch.randn(geo.nwall, geo.nr, generator=torch.Generator().manual_seed(5))
    ref = VO.reference(VO.params_of_model(model), geo, "cuda", "noocl", k["c"] * k["deltaT"], 5.7, gout)
    dead = torch.nonzero(ref.scale["scaling"] == 0).flatten()
    assert dead.numel() > 0
    g = int(dead[0])
    got = {n: t.clone() for n, t in ref.grads.items()}
    assert VO.unreached_failures(got, ref) == []
    got["scaling"][g, 0] += 2.0 * float(ref.bracket["scaling"][g]) + 1e-12
    assert [(b[0], b[1]) for b in VO.unreached_failures(got, ref)] == [("scaling", g)]
    assert [(b[0], b[1]) for b in VO.failures(got, ref, 2e-4)] == [("scaling", g)]


def test_as_named_splits_the_flat_feature_gradient():
    ng, K = 5, 16
    five = [torch.randn(ng, 3), torch.randn(ng, 3), torch.randn(ng, 4), torch.randn(ng), torch.randn(ng, K)]
    d = VO.as_named(five)
    assert [tuple(d[n].shape) for n in VO.NAMES] == [(ng, 3), (ng, 3), (ng, 4), (ng, 1), (ng, 1), (ng, K - 1)]
    assert torch.equal(d["features_dc"][:, 0], five[4][:, 0].double())
    assert torch.equal(d["features_rest"], five[4][:, 1:].double())


# ---------------------------------------------------------------------------------------------------------
# the per-bin forward metric
# ---------------------------------------------------------------------------------------------------------
CUT = 5.7


def _bins(model, geo, k, preset, mode, cutoff=CUT):
    P = VO.params_of_model(model)
    cdt = k["c"] * k["deltaT"]
    fb = VO.forward_bins(P, geo, preset, mode, cdt, cutoff)
    return P, cdt, fb


@pytest.mark.parametrize("preset", ["torch", "cuda"])
@pytest.mark.parametrize("mode", ["noocl", "netf"])
@pytest.mark.parametrize("T,ns", [(41, 6), (97, 6), (97, 8), (257, 8), (0, 6)])
def test_fp32_oracle_passes_the_per_bin_metric(preset, mode, T, ns):
    """(a) Scene 1 (T = 0: its compact variant): another fp32 evaluation of the same sums is within 2e-5 of every
    bin's own scale (Q = 0)."""
    model, geo, k = VO.parity_scene(preset, mode, T, ns=ns) if T else VO.compact_scene(preset, mode, ns=ns)
    P, cdt, fb = _bins(model, geo, k, preset, mode)
    with torch.no_grad():
        hist = R.render_volume(P, k["walls"], k["box"], k["Y"], k["ns"], k["start"], k["end"], k["c"], k["deltaT"],
                               preset=preset, mode=mode, mc=CUT)
    tol = VO.forward_tolerance(P, geo, preset, CUT, base=2e-5)
    w = VO.forward_bin_worst(hist, fb)
    print(f"\n{preset} {mode} T={T} ns={ns}: fp32 oracle per bin {w:.2e}, per row "
          f"{VO.forward_worst(hist, VO.as_row_reference(fb)):.2e}")
    assert VO.forward_bin_failures(hist, fb, tol) == []
    assert VO.forward_bin_failures(fb.ref, fb, 0.0) == [] and VO.forward_bin_worst(fb.ref, fb) == 0.0


def test_per_bin_metric_rejects_single_ray_faults():
    """(b) Scene 1, compact (volume_oracle.compact_scene: cuda, noocl, T = 97, ns = 6; about 1700 rays per wall
    point, rows with structure).  Each fault changes one ray of one Gaussian at wall point 0 in the float64
    reference: drained one bin late; its last in-support bin dropped; left out; added twice (the ray after it in
    its row, as a pair whose second ray is drained again).  The bound uses the coarsest unit the quantile rule can
    pick (coarsest_E) and FWD_BIN_TOL with the position allowance.  The two figures are computed for every
    (Gaussian, ray), and the example is the ray on which the per-bin metric rejects the first two faults most
    clearly among those where 2e-5 of the row maximum, the earlier forward tests' figure, passes both: the gap this
    metric closes.  (On the broad scene 1 the rows are flat, every bin is near its row's maximum, and the two
    figures reject the same rays.)  Over all rays the per-bin metric at the coarsest unit rejects somewhat fewer
    planted faults than 2e-5 of the row maximum: its gain is the independent reference and the bins away from the
    row's peak, not a uniformly sharper rule."""
    model, geo, k = VO.compact_scene()
    P, cdt, fb = _bins(model, geo, k, "cuda", "noocl")
    tol = VO.forward_tolerance(P, geo, "cuda", CUT)
    E = VO.coarsest_E(P, "cuda", "noocl", cdt)
    row = VO.as_row_reference(fb)
    with torch.no_grad():
        t = VO.ray_terms(VO.Params64(P), VO.tables(geo), 0, "cuda", "noocl", cdt, CUT)      # [Ng, nr, rays]
    ng, nr, nray = t.shape
    ta, b, q = VO._bin_bound(fb, tol, E)
    bound, top = (ta + b + q)[0], fb.ref[0].max()
    late = torch.zeros_like(t)
    late[:, 1:] = t[:, :-1]
    klast = ((t > 0) * torch.arange(nr)[None, :, None]).amax(dim=1, keepdim=True)            # [Ng, 1, rays]
    last = torch.zeros_like(t).scatter_(1, klast, t.gather(1, klast))
    deltas = {"one bin late": late - t, "last bin dropped": -last, "left out": -t,
              "second ray of a pair twice": torch.roll(t, -1, dims=2)}
    hit = (t > 0).any(dim=1)
    figs = {}
    for name, d in deltas.items():
        figs[name] = ((d.abs() / bound[None, :, None]).amax(dim=1), d.abs().amax(dim=1) / top)   # [Ng, rays] each
        print(f"\n{name}: of the {int(hit.sum())} (Gaussian, ray) in support the per-bin metric rejects "
              f"{int((figs[name][0] > 1)[hit].sum())}, 2e-5 of the row maximum "
              f"{int((figs[name][1] > 2e-5)[hit].sum())}, "
              f"the per-bin metric alone {int(((figs[name][0] > 1) & (figs[name][1] <= 2e-5))[hit].sum())}")
    # floors, so that the scene cannot drift into one where the metric sees little: at the coarsest unit it rejects
    # more than half of the rays drained a bin late and two thirds of the rays left out (measured 787 and 1024 of
    # 1511; 2e-5 of the row maximum 886 and 1142), and some of each fault that the row figure passes
    nhit = int(hit.sum())
    assert int((figs["one bin late"][0] > 1)[hit].sum()) > 0.5 * nhit
    assert int((figs["left out"][0] > 1)[hit].sum()) > 0.65 * nhit
    assert all(int(((f[0] > 1) & (f[1] <= 2e-5))[hit].sum()) > 0 for f in figs.values())
    f1, f2 = figs["one bin late"], figs["last bin dropped"]
    ok = hit & (f1[1] <= 2e-5) & (f2[1] <= 2e-5) & (torch.arange(nray) % geo.np < geo.np - 1)[None, :]
    score = torch.where(ok, torch.minimum(f1[0], f2[0]), torch.zeros_like(f1[0]))
    g, ray = divmod(int(score.argmax()), nray)
    passed_by_row = []
    for name, d in deltas.items():
        faulty = fb.ref.clone()
        faulty[0] += d[g, :, ray]
        bad = VO.forward_bin_failures(faulty, fb, tol, E)
        rw, bw = VO.forward_worst(faulty, row), VO.forward_bin_worst(faulty, fb, E)
        print(f"Gaussian {g} ray {ray}, {name}: {rw:.2e} of the row maximum (the old figure), {bw:.2e} of the bin's "
              f"own scale beyond B + Q (tolerance {float(tol[g]):.2e}); {len(bad)} bins fail")
        assert bad and all(f[0] == 0 for f in bad), name
        passed_by_row.append(rw <= 2e-5)
    assert passed_by_row[0] and passed_by_row[1], passed_by_row
    assert VO.forward_bin_failures(fb.ref, fb, tol, E) == []


def _coverage_scenes():
    """(name, (model, geo, consts), preset, mode, held): every scene family of tests/test_gpu_fwd_edges.py, built by
    that file's own builders; held = False for the exempt ones."""
    import test_gpu_fwd_edges as FE
    yield "1 cuda noocl T=97", VO.parity_scene("cuda", "noocl", 97), "cuda", "noocl", True
    yield "1 torch netf T=257", VO.parity_scene("torch", "netf", 257, ns=8), "torch", "netf", True
    yield "1 cuda netf T=97 ns=8", VO.parity_scene("cuda", "netf", 97, ns=8), "cuda", "netf", True
    yield "1 compact noocl", VO.compact_scene(), "cuda", "noocl", True
    yield "1 compact netf", VO.compact_scene(mode="netf"), "cuda", "netf", True
    for L in (19, 36, 72):
        model, geos, k = FE._one_gaussian(L, "noocl", 40)
        yield f"2 one Gaussian L={L}", (model, geos[0], k), "cuda", "noocl", False
    for T in (7, 17, 35):
        yield f"3 short rows T={T}", FE._short_row_scene(T, "noocl", None)[:3], "cuda", "noocl", True
    for ns in (5, 16):
        yield f"4 runs ns={ns}", VO.runs_scene(ns), "cuda", "noocl", True
    for ng in (1, 2, 65, 257, 2049):
        yield f"5 lanes ng={ng}", VO.lanes_scene(ng, 3), "cuda", "noocl", True
    yield "5 lanes ng=513 netf", VO.lanes_scene(513, 5, mode="netf"), "cuda", "netf", True
    yield "6 needles", FE._needle_scene("noocl", None), "cuda", "noocl", False
    for mode in ("noocl", "netf"):
        yield f"6 thin axis {mode}", FE._thin_scene(mode, None), "cuda", mode, True
        yield f"6 sub-bin {mode}", FE._sub_bin_scene(mode, None), "cuda", mode, True
    for nb in (0, 1, 2, 3, 30):
        yield f"7 bright {nb}", VO.bright_scene(nb), "cuda", "noocl", nb <= 1
    yield "7 flush pile", VO.pile_scene(), "cuda", "noocl", True


def test_bracket_and_rounding_do_not_decide_most_bins():
    """(c) Per scene, of the bins with ref > 0 at most a quarter have B + Q > 10 sum_g tol_g (A_g + B_g).  E is the
    coarsest the scene allows, except for scene 7, whose point is the unit the quantile rule picks (quantile_E; the
    GPU test asserts the kernel's E equals it).  Every scene family of tests/test_gpu_fwd_edges.py is printed; held
    to the quarter are all but three, which are exempt for the reason given and listed with their measured fraction:
      scene 2 (0.22 to 0.32)  one Gaussian alone: the bins at its own edge hold only samples beyond 4 sigma
      6 needles (0.26)        each crossing is a single ray's profile; its flank bins are below the rounding bound
                              of the wall point's hundred rays (0.24 to 0.34 for other placements of the needles)
      7 bright 2, 3, 30       (0.73, 0.66, 0.56) the unit is coarsened on purpose: Q is what the case is about
    Scene 6 (thin axis, sub-bin) and the pile meet it with equally bright Gaussians of a tight amplitude bound
    (volume_oracle.tight_albedo) and, for the pile, a row cut to its core."""
    worst = 0.0
    for name, (model, geo, k), preset, mode, held in _coverage_scenes():
        P, cdt, fb = _bins(model, geo, k, preset, mode)
        E = VO.quantile_E(P, preset, mode, cdt, geo.nt * geo.np)[0] if name.startswith("7 bright") \
            else VO.coarsest_E(P, preset, mode, cdt)
        c = VO.forward_bin_coverage(fb, VO.forward_tolerance(P, geo, preset, CUT), E)
        print(f"\n{name}: E {E:.2f}, {int((fb.ref > 0).sum())} of {fb.ref.numel()} bins live, bracket or rounding "
              f"decides in {c:.3f} of them" + ("" if held else "  (exempt)"))
        if held:
            worst = max(worst, c)
    assert worst <= 0.25


@pytest.mark.parametrize("ng", [1, 2, 63, 64, 65, 255, 256, 257, 513, 2049])
def test_lanes_scene_every_gaussian_stands_out(ng):
    """Scene 5: a Gaussian lost at a chunk or split boundary fails a bin outright: every Gaussian (above 65: every
    one at a chunk boundary, the others are dimmed) has a bin in which its A_g is more than ten times the bin's
    whole bound, at the coarsest unit."""
    model, geo, k = VO.lanes_scene(ng, 3)
    P, cdt, fb = _bins(model, geo, k, "cuda", "noocl")
    ta, b, q = VO._bin_bound(fb, VO.forward_tolerance(P, geo, "cuda", CUT), VO.coarsest_E(P, "cuda", "noocl", cdt))
    stand = (fb.A_g / (ta + b + q).clamp_min(1e-300)[:, None, :]).amax(dim=(0, 2))
    share = (fb.A_g / fb.A.clamp_min(1e-300)[:, None, :]).amax(dim=(0, 2))
    sel = VO.lane_boundary(ng) if ng > 65 else torch.ones(ng, dtype=torch.bool)
    print(f"\nng={ng}: {int(sel.sum())} Gaussians checked, least A_g / bound {float(stand[sel].min()):.1f}, least best "
          f"share of a bin {float(share[sel].min()):.3f}")
    assert float(stand[sel].min()) > 10.0


def test_quantile_rule_of_the_bright_scene():
    """Scene 7: 300 Gaussians, so the second brightest bound sets the unit: one bright Gaussian leaves it alone
    (the bright launch carries it), two or more coarsen it to the unit of the bright bounds (7 binary orders)."""
    E = {}
    for nb in (0, 1, 2, 3, 30):
        model, geo, k = VO.bright_scene(nb)
        E[nb] = VO.quantile_E(VO.params_of_model(model), "cuda", "noocl", k["c"] * k["deltaT"], geo.nt * geo.np)
    print("\n(E, E of the largest bound) per number of bright Gaussians:", E)
    assert E[1][0] == E[0][0] and E[1][1] <= E[1][0] - 6
    assert all(E[nb][0] == E[nb][1] == E[1][1] for nb in (2, 3, 30))


# ---------------------------------------------------------------------------------------------------------
# per-ray outputs, the per-ray upstream, occlusion and AABB selection
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,selection,cutoff,opaque", [
    ("occl", "support", 0.0, True), ("occl", "support", 0.0, False), ("occl", "support", 5.7, True),
    ("occl", "aabb", 0.0, False), ("occl", "aabb", 5.7, False), ("noocl", "aabb", 0.0, False), ("noocl", "aabb", 5.7, False)])
def test_occl_and_aabb_forward_match_fp32_oracle(mode, selection, cutoff, opaque):
    """The float64 occl / aabb forward against fp32 render_rays_cuda and aabb_filter (pinned to the reference's golden
    files by test_oracle_golden.py) on a 24-Gaussian scene of 9 x 5 rays and 40 bins, with the T < 1e-4 cut reached
    (opaque: dead samples exist, and are zero in both) and not: every (ray, bin) within 1e-5 of the tensor's maximum,
    the rounding of an fp32 sum of 24 terms and of exp (measured: 4e-7); the per-ray lists are identical."""
    model, geo, cdt = VO.ladder_scene(40, mode=mode, selection=selection)
    if not opaque:
        with torch.no_grad():
            model._opacity.sub_(3.0)
    bb = VO.boxes_of(model) if selection == "aabb" else None
    P = VO.params_of_model(model)
    rs = cdt if mode == "noocl" else 1.0
    hist, rays, T, sels = VO.forward_rays(P, geo, "cuda", mode, cdt, cutoff, selection, bb, ray_scale=rs)
    _, ref32, _, lists = VO.fp32_oracle(model, geo, mode, cdt, cutoff, selection, bb, ray_scale=rs)
    if mode == "occl":
        assert bool((T < 1e-4).any()) == opaque
        dead = T.transpose(1, 2) < 1e-4
        assert float(rays[dead].abs().sum()) == 0.0 and float(ref32[dead].abs().sum()) == 0.0
        assert bool((ref32[~dead] > 0).any())
    if selection == "aabb":
        for p, filt in enumerate(lists):
            mask = torch.zeros_like(sels[p])
            for ray in range(filt.shape[0]):
                mask[filt[ray, 1:1 + int(filt[ray, 0])].long(), ray] = True
            assert torch.equal(mask, sels[p])
        assert 0.0 < float(torch.stack(sels).double().mean()) < 1.0
    err = float((rays - ref32.double()).abs().max() / rays.abs().max())
    print(f"\n{mode} {selection} cutoff={cutoff} opaque={opaque}: fp32 oracle rays {err:.2e} of the maximum")
    assert err <= 1e-5


def test_aabb_cap_keeps_the_first_256_by_index():
    """300 boxes that cover every ray: each ray keeps Gaussians 0..255."""
    model, geo, cdt = VO.window_scene(300, mode="occl", scale_shift=2.5)
    sel = VO.selection_mask(VO.tables(geo), 0, VO.boxes_of(model))
    assert bool(sel[:256].all()) and not bool(sel[256:].any())


@pytest.mark.parametrize("mode,selection", [("noocl", "support"), ("netf", "support"), ("occl", "support"),
                                            ("occl", "aabb"), ("noocl", "aabb")])
def test_rays_sum_to_the_histogram(mode, selection):
    """hist[p, k] = hscale[p] att[k] sum_rays sin(theta) rays[p, ray, k] / ray_scale."""
    model, geo, cdt = VO.ladder_scene(65, mode=mode, selection=selection)
    bb = VO.boxes_of(model) if selection == "aabb" else None
    ref = VO.reference(VO.params_of_model(model), geo, "cuda", mode, cdt, 5.7, None, None, selection, bb, ray_scale=0.37)
    tab = VO.tables(geo)
    st = tab["st"][:, :, None].expand(-1, -1, geo.np).reshape(geo.nwall, -1)
    h = tab["hscale"][:, None] * tab["att"][None, :] * (ref.rays * st[:, :, None]).sum(dim=1) / 0.37
    assert float(ref.hist.abs().max()) > 0
    assert float((h - ref.hist).abs().max()) <= 1e-12 * float(ref.hist.abs().max())
    assert all(float(g.abs().max()) == 0.0 for g in ref.grads.values())     # no upstream: no gradient


@pytest.mark.parametrize("mode,selection,cutoff", [("netf", "support", 5.7), ("occl", "support", 0.0), ("occl", "aabb", 5.7)])
def test_one_hot_gray_is_the_gradient_of_that_sample(mode, selection, cutoff):
    """gout = None and a one-hot gray: the gradients equal torch autograd of the single sample rays[p, ray, k]."""
    model, geo, cdt = VO.ladder_scene(40, mode=mode, selection=selection)
    bb = VO.boxes_of(model) if selection == "aabb" else None
    p, ray, k = 1, 3 * geo.np + 2, 17
    gray = torch.zeros(geo.nwall, geo.nt * geo.np, geo.nr)
    gray[p, ray, k] = 1.0
    ref = VO.reference(VO.params_of_model(model), geo, "cuda", mode, cdt, cutoff, None, gray, selection, bb, ray_scale=0.5)
    P = VO.Params64(VO.params_of_model(model))
    tab = VO.tables(geo)
    sel = VO.selection_mask(tab, p, bb) if bb is not None else None
    out, _ = VO.ray_outputs(P, tab, p, "cuda", mode, cdt, cutoff, sel)
    sample = 0.5 * out[k, ray]
    assert float(sample.detach()) > 0 and float(sample.detach()) == float(ref.rays[p, ray, k])
    want = torch.autograd.grad(sample, P.leaves(), allow_unused=True)
    for n, w in zip(VO.NAMES, want):
        w = torch.zeros_like(ref.grads[n]) if w is None else w.reshape(ref.grads[n].shape)
        assert float((ref.grads[n] - w).abs().max()) <= 1e-12 * max(float(w.abs().max()), 1e-300), n
        assert bool((ref.scale[n] >= ref.grads[n].abs().amax(dim=1) * (1 - 1e-12)).all())


def test_reference_is_linear_in_both_upstreams():
    """grad(a gout1 + b gout2, a gray1 + b gray2) = a grad(gout1, gray1) + b grad(gout2, gray2); and the hist upstream
    that a gray reproduces (gray = gout att hscale sin(theta) / ray_scale) gives the same gradient."""
    model, geo, cdt = VO.ladder_scene(40)
    Pm = VO.params_of_model(model)
    g = torch.Generator().manual_seed(3)
    go = [torch.randn(geo.nwall, geo.nr, generator=g).double() for _ in range(2)]
    gr = [torch.randn(geo.nwall, geo.nt * geo.np, geo.nr, generator=g).double() for _ in range(2)]
    f = lambda a, b: VO.reference(Pm, geo, "cuda", "occl", cdt, 5.7, a, b, ray_scale=0.5)
    r1, r2, r12 = f(go[0], gr[0]), f(go[1], gr[1]), f(2.0 * go[0] - 3.0 * go[1], 2.0 * gr[0] - 3.0 * gr[1])
    for n in VO.NAMES:
        want = 2.0 * r1.grads[n] - 3.0 * r2.grads[n]
        assert float((r12.grads[n] - want).abs().max()) <= 1e-11 * float(r12.scale[n].max()), n
    eq = VO.equivalent_gray(geo, go[0], 0.5)
    a, b = f(go[0], None), f(None, eq)
    for n in VO.NAMES:
        assert float((a.grads[n] - b.grads[n]).abs().max()) <= 1e-12 * float(a.scale[n].max()), n
        assert float((a.scale[n] - b.scale[n]).abs().max()) <= 1e-12 * float(a.scale[n].max()), n


def _margin_cases():
    """(name, model, geo, mode, c dT, cutoff, selection): every scene of test_gpu_ray_upstream.py's tile part and of
    test_gpu_tile_edges.py at every parameter value they use (the pair-major scenes hold no discontinuous decision)."""
    import test_gpu_ray_upstream as RU
    import test_gpu_tile_edges as TE
    for name, (model, geo, cdt), mode, cutoff, selection in list(RU.margin_cases()) + list(TE.margin_cases()):
        yield name, model, geo, mode, cdt, cutoff, selection


def test_decision_margins_of_every_gpu_scene():
    """Every T_k stays 1e-3 (relative) away from 1e-4 and every slab time 1e-3 of the ray's length away from its
    decision, in every scene the two GPU files judge against this reference.  A seed that fails is changed in the
    scene builder; the 1e-3 stays."""
    worst = {"T": float("inf"), "slab": float("inf")}
    for name, model, geo, mode, cdt, cutoff, selection in _margin_cases():
        bb = VO.boxes_of(model) if selection == "aabb" else None
        m = VO.decision_margins(VO.params_of_model(model), geo, "cuda", mode, cdt, cutoff, selection, bb)
        print(f"\n{name}: T {m['T']:.2e}, slab {m['slab']:.2e}")
        assert m["T"] > 1e-3 and m["slab"] > 1e-3, (name, m)
        worst = {k: min(worst[k], m[k]) for k in worst}
    print("\nsmallest margins:", worst)


def test_opaque_scene_cuts_in_every_chunk():
    """opaque_scene: by the float64 reference the first dead bin lies in chunk 0 for some rays, in a later chunk for
    others and nowhere for at least one, at both row lengths."""
    for nr in (97, 257):
        model, geo, cdt = VO.opaque_scene(nr)
        T = VO.forward_rays(VO.params_of_model(model), geo, "cuda", "occl", cdt, 0.0)[2]
        fd = VO.first_dead_bin(T)
        assert bool((fd < 64).any()) and bool(((fd >= 64) & (fd < nr)).any()) and bool((fd == nr).any()), fd


def test_walk_scene_has_every_class_in_a_sorted_block():
    """walk_scene: at cutoff 5.0 and 5.7 some block of 64 entries x 4 rays holds more than 64 live pairs (the sorted
    order) of all four length classes, and walks longer than 200 bins exist."""
    model, geo, cdt = VO.walk_scene()
    assert cdt <= 1.0 / 64
    for cutoff in (5.0, 5.7):
        L = VO.walk_lengths(model, geo, cutoff)
        blocks = [b for p in range(geo.nwall) for b in VO.walk_blocks(L, p, 8, 4)]
        assert any(n > 64 and c == [0, 1, 2, 3] for n, c in blocks)
        assert int((L > 200).sum()) > 0
        for lo, hi in ((1, 28), (28, 56), (56, 96), (96, 200)):
            assert int(((L >= lo) & (L < hi)).sum()) > 0
