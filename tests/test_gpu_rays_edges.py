"""Per-element float64 parity of the path-C rays API (csrc/nlosgr_rays.hip: filter_kernel, rays_fwd_kernel,
rays_bwd_kernel, rays_finish_kernel) at its kernels' edges.

Every case calls nlosgr.rays.rays_forward / rays_backward (or the C ABI) directly and compares with the float64
reference of tests/rays_oracle.py: the three outputs ray by ray (max_s |hip - ref| <= FWD_TOL max_s |ref|), the five
gradient tensors Gaussian by Gaussian (e_g <= TOL[tensor] s_g with the cancellation-aware scale s_g), and with `==`
what must be exact: a dead sample (T_s < 1e-4) is 0 in all three outputs, T is 1 without occlusion, a ray with an
empty row gives 0, 0 and 1 (with occlusion too), a Gaussian no filter row names gets zero in all five gradient
tensors.  The filter rows are an input shared by the kernel and the reference.  Every occlusion scene asserts its
float64 decision margin min |T_s / 1e-4 - 1| >= 1e-3, so no sample is left out.

Scenes (rays_oracle.py; both presets, with and without occlusion, SH degrees 0 to 3 spread over the four):
  A  nsamp 1, 63, 64, 65, 129, 200 on a non-uniform t; ray 0's first dead sample at lane 63 of chunk 0, lane 0 of
     chunk 1, lane 0 of chunk 2, inside chunk 2; a ray that names one Gaussian and never dies; 5 rays (4 + 1)
  B  rows of 0, 1, 64, 65 and 256 Gaussians out of 300 (3 rays, 1 ray); the unnamed ones (44 of 300 under the 256-row) exactly zero
  C  1030 rays: backward slots 0 to 5 take two rays each, empty row first or second; run twice, bitwise equal
  D  g_rho / g_density / g_trans alone and together, one-hot upstreams at samples 0, 63, 64, nsamp - 1, 1e6 on every
     dead sample changes no bit; one case with 16 feature columns at SH degree 1
  E  nsamp = 8192 (104 KiB of dynamic LDS in the backward), 2 rays, 3 broad Gaussians
  F  the filter, bit-exact against oracle.torch_ref.aabb_filter: ng 0, 1, 63, 64, 65, 129 x nrays 1, 3, 5; the 256th
     hit inside a 64-Gaussian block; directions with a component exactly 0 and negative components, an origin
     inside a box, a box behind the origin, a ray that hits nothing
  G  empty sizes and invalid arguments through the C ABI

The tolerances.  TOL and FWD_TOL are 8 times the worst value of the fp32 oracle (rays_oracle.fp32_oracle: the same
sums in fp32 with torch autograd, measured on the CPU) over scenes A, B and D, rounded up to one significant digit;
the factor covers what that oracle lacks (the hardware exp2, the butterfly reduction order, the per-slot summation
order).  None exceeds what test_gpu_rays.py promises per tensor (forward 2e-5, 2e-4 with occlusion; gradients 2e-4,
3e-4 with occlusion): the forward rho without occlusion would be 3e-5 and is capped at 2e-5.  The oracle is taken
in its expm1 form; oracle.torch_ref.render_rays_cuda itself forms alpha as 1 - exp(-x), which in fp32 cancels to
6e-8 absolute and puts a feature row made of small alphas off by 53 % (scene B) and a ray's rho by 1e-4: never the
narrower of the two, so the tolerances below are at most what the literal recipe gives.  The kernel's values are
printed by pytest -s and never feed a tolerance.  Worst values ((e_g)/s_g per tensor, the forward per ray):

    fp32 oracle (CPU)          mu   scaling  rotation   opacity   feat_dc feat_rest |     rho   density     trans
    A  no occlusion       6.5e-07   3.5e-07   3.0e-06   4.6e-07   2.2e-07   7.3e-08 | 3.6e-06   3.6e-07         0
    A  occlusion          3.4e-07   3.3e-07   3.1e-06   4.1e-07   2.4e-07   2.5e-07 | 2.6e-06   3.6e-07   1.0e-07
    B  no occlusion       1.4e-06   1.3e-06   6.9e-06   1.5e-06   2.8e-06   4.3e-08 | 2.1e-06   1.0e-06         0
    B  occlusion          2.8e-06   2.9e-06   9.0e-06   3.0e-06   2.9e-06   3.0e-06 | 1.3e-06   1.0e-06   1.1e-07
    D  no occlusion       7.4e-07   6.3e-07   1.2e-05   9.0e-07   8.1e-07   8.7e-07 | 5.0e-07   2.9e-07         0
    D  occlusion          9.5e-07   8.6e-07   5.0e-06   7.4e-07   1.1e-06   1.2e-06 | 5.3e-07   2.9e-07   9.1e-08
    TOL (8 x worst)         3e-05     3e-05     1e-04     3e-05     3e-05     3e-05 | 2e-05 (occlusion 3e-05)  9e-06  9e-07
    (C and E, not part of the tolerance: at most 9.2e-08 per tensor, 7.5e-07 forward)

    kernel (MI355X)            mu   scaling  rotation   opacity   feat_dc feat_rest |     rho   density     trans
    A  no occlusion       3.5e-07   4.2e-07   5.3e-06   3.0e-07   4.8e-07   1.6e-07 | 3.6e-06   2.5e-07         0
    A  occlusion          3.6e-07   4.3e-07   4.7e-06   3.5e-07   5.0e-07   4.6e-07 | 2.5e-06   2.5e-07   8.8e-08
    B  no occlusion       1.9e-06   1.8e-06   5.5e-05   1.8e-06   2.0e-06   4.1e-08 | 2.1e-06   7.5e-07         0
    B  occlusion          3.0e-06   3.2e-06   4.9e-05   3.2e-06   3.3e-06   3.4e-06 | 1.1e-06   7.5e-07   1.3e-07
    C  no occlusion       1.3e-08   4.0e-09   1.4e-07   4.9e-09   9.5e-09   5.3e-09 | 6.1e-07   3.1e-07         0
    C  occlusion          2.3e-08   7.4e-09   2.1e-07   9.6e-09   4.6e-08   6.0e-08 | 3.8e-07   3.1e-07   1.0e-07
    D  no occlusion       6.4e-07   7.4e-07   6.7e-06   7.5e-07   7.1e-07   2.3e-07 | 4.9e-07   2.3e-07         0
    D  occlusion          6.3e-07   8.3e-07   7.2e-06   8.2e-07   1.1e-06   1.2e-06 | 4.0e-07   2.3e-07   7.5e-08
    E  no occlusion       1.4e-08   1.2e-08   6.1e-08   5.1e-09   7.2e-09   4.9e-09 | 6.2e-07   1.5e-07         0
    E  occlusion          6.3e-09   1.0e-08   4.3e-08   3.5e-08   1.6e-08   1.6e-08 | 8.4e-07   1.4e-07   1.2e-07

The kernel stays within every tolerance on every scene; its worst margin is a factor 1.8 (d_rotation on the
256-Gaussian rows of scene B, 5.5e-05 against 1e-04), everywhere else 5 and more.

Found by these tests and fixed in csrc/nlosgr_rays.hip with them:
  1. nlosgr_rays_bwd refused nrays = 0 with NLOSGR_E_INVALID ("workspace/filter is null") when the filter pointer was
     NULL, which is what an empty [0, 257] tensor has; no ray needs no row, and the call must return zero gradients.
     The filter is now required only when nrays > 0 (scene G, test_abi_no_rays).
Measured and found in order, no change needed:
  2. The backward's launch at nsamp = 8192 asks for 104 KiB of dynamic LDS and no kernel raises a dynamic-LDS limit.
     On gfx950 the HIP runtime admits a launch up to the device's 160 KiB per workgroup without an opt-in (the
     function attribute for it exists for source compatibility); scene E launches, and its forward and all five
     gradient tensors are within tolerance for both presets and both occlusion modes.
  3. The slot loop (scene C), the scans' chunk carries (scenes A, D and E), full LDS staging (scene B), the NULL
     upstream branches and the dead samples' upstream (scene D), the torch preset (every scene) and the filter's cap
     inside a block (scene F) agree with the reference as they are.

Mutation check (by hand on a copy of csrc/, not committed): `carry += __shfl(incl, 62)` instead of lane 63 fails scene A
(nsamp 65, 129 and 200 under occlusion, both presets); the suffix scan's `lane + off <= 64` instead of `< 64` fails
scene D (g_rho, g_trans and all three under occlusion, the one-hot at sample 63).  Dropping the wave_sync() at the
top of the slot loop changes no result of scene C: a backward workgroup is one wave, whose LDS operations execute in
program order, so that barrier only keeps the compiler from moving the next ray's staging stores above the previous
ray's reads; scene C pins the loop's arithmetic (two rays added into one row, `continue` first or second), not that
ordering.
"""
import pytest
import torch

from conftest import ROOT  # noqa: F401

import rays_oracle as RO
import volume_oracle as VO

pytestmark = pytest.mark.gpu

TOL, FWD_TOL = RO.TOL, RO.FWD_TOL   # 8 x the fp32 oracle's worst value over scenes A, B and D (module docstring)

PRESETS = ("cuda", "torch")
_TABLE = {}   # (scene, occl) -> {tensor or output: the kernel's worst value}


@pytest.fixture(scope="module", autouse=True)
def _print_table():
    yield
    cols = list(VO.NAMES) + list(RO.OUTPUTS)
    print("\n\nkernel: worst measured value per scene (per Gaussian; the forward per ray)\n"
          + f"{'scene':<22}" + "".join(f"{c[:9]:>10}" for c in cols))
    for (scene, occl), row in sorted(_TABLE.items()):
        print(f"{scene + ('  occlusion' if occl else '  no occlusion'):<22}"
              + "".join(f"{row.get(c, 0.0):>10.1e}" for c in cols))


def _dev():
    return torch.device("cuda:0")


def _launch(sc, ups, forward=True):
    """(rho, density, T) and the five gradient tensors of the HIP kernels for a rays_oracle.Scene."""
    from nlosgr.rays import rays_backward, rays_forward
    dev = _dev()
    P = sc.P
    args = [x.detach().to(dev).contiguous() for x in (sc.o, sc.d, sc.t, P._mu, P._scaling, P._rotation, P._opacity,
                                                       sc.feats, sc.cam)]
    args += [sc.deg, sc.cdt, 1.0, sc.occl, sc.filt.to(dev).contiguous()]
    fwd = rays_forward(*args, preset=sc.preset) if forward else None
    g = [None if u is None else u.to(dev).float().contiguous() for u in ups]
    return fwd, rays_backward(*args, *g, preset=sc.preset)


def _exact_forward(sc, fwd, ref):
    rho, dens, tr = (x.cpu() for x in fwd)
    empty = sc.filt[:, 0] == 0
    if not sc.occl:
        assert bool((tr == 1.0).all()), "T must be exactly 1 without occlusion"
    dead = ref.dead
    for name, x in (("rho", rho), ("density", dens), ("trans", tr)):
        assert bool((x[dead] == 0.0).all()), f"a dead sample is not exactly 0 in {name}"
    assert bool((tr[~dead] > 0.0).all()), "a live sample came out dead"
    assert bool((rho[empty] == 0.0).all()) and bool((dens[empty] == 0.0).all()) and bool((tr[empty] == 1.0).all()), \
        "a ray with an empty row must give exactly 0, 0 and 1"
    assert bool((ref.trans[empty] == 1.0).all())      # the reference agrees: nothing occludes such a ray


def _exact_backward(grads, ref):
    unnamed = ~ref.named
    for name, g in zip(("d_mu", "d_scaling", "d_rotation", "d_opacity", "d_features"), grads):
        g = g.cpu().reshape(unnamed.shape[0], -1)
        assert bool((g[unnamed] == 0.0).all()), f"{name}: a Gaussian no filter row names is not exactly zero"


def _check(scene, case, sc, ups, ref=None, forward=True):
    """Forward and backward against the reference; prints and records the worst values, then asserts."""
    ref = sc.reference(ups) if ref is None else ref
    if sc.occl:
        assert ref.margin >= RO.MARGIN, f"decision margin {ref.margin:.2e}"
    fwd, grads = _launch(sc, ups, forward)
    named = VO.as_named(grads)
    worst = VO.worst(named, ref)
    fw = RO.forward_worst(fwd, ref) if forward else {}
    print(f"\n{scene} {case}: " + ", ".join(f"{n} {v:.2e}" for n, v in list(fw.items()) + list(worst.items())))
    row = _TABLE.setdefault((scene, sc.occl), {})
    for n, v in list(worst.items()) + list(fw.items()):
        row[n] = max(row.get(n, 0.0), v)
    for g in grads:
        assert bool(torch.isfinite(g).all())
    if forward:
        _exact_forward(sc, fwd, ref)
        for n, v in fw.items():
            assert v <= FWD_TOL[sc.occl][n], f"forward {n}: {v:.3e} of a ray's maximum, tolerance {FWD_TOL[sc.occl][n]:.1e}"
    _exact_backward(grads, ref)
    bad = VO.failures(named, ref, TOL)
    assert not bad, f"{len(bad)} (tensor, Gaussian, e_g, s_g, b_g) beyond tolerance, first: {bad[:6]}"
    return fwd, grads, ref


# ---------------------------------------------------------------------------------------------------------
# A. sample counts and the scans across 64-sample chunks
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occl", [False, True])
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("nsamp", RO.A_NSAMP)
def test_sample_counts(nsamp, preset, occl):
    """nsamp 1, 63, 64, 65, 129, 200 (5 rays: not a multiple of the 4 rays of a forward workgroup); under occlusion
    ray 0's first dead sample sits where rays_oracle.A_FIRST_DEAD puts it (test_rays_oracle_cpu.py pins it)."""
    sc = RO.scene_A(nsamp, preset, occl)
    ups = sc.upstreams()
    ref = sc.reference(ups)
    if occl and RO.A_FIRST_DEAD[nsamp] is not None:
        assert ref.first_dead()[0] == RO.A_FIRST_DEAD[nsamp] and ref.first_dead()[4] == -1
    _check("A sample counts", f"nsamp={nsamp} {preset} occl={occl}", sc, ups, ref)


# ---------------------------------------------------------------------------------------------------------
# B. selected counts: 0, 1, 64, 65, 256 staged Gaussians
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occl", [False, True])
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("counts", RO.B_COUNTS, ids=lambda c: "-".join(map(str, c)))
def test_selected_counts(counts, preset, occl):
    """Rows of 0, 1, 64, 65 and 256 of 300 Gaussians (stage_ray's lane loop, the full LDS table), 3 rays and 1 ray;
    every Gaussian no row names must come out exactly zero."""
    sc = RO.scene_B(counts, preset, occl)
    assert sc.filt[:, 0].tolist() == list(counts)
    ups = sc.upstreams()
    ref = sc.reference(ups)
    unnamed = int((~ref.named).sum())
    assert unnamed >= max(RO.B_NG - sum(counts), 30) and (counts != (256,) or unnamed == 44)
    _check("B selected counts", f"counts={counts} {preset} occl={occl}", sc, ups, ref)


# ---------------------------------------------------------------------------------------------------------
# C. more than one ray per backward slot
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occl", [False, True])
@pytest.mark.parametrize("preset", PRESETS)
def test_two_rays_per_slot(preset, occl):
    """1030 rays on 1024 slots: the slot loop, its wave_sync before the LDS tables are reused, the add into a row
    that already holds a ray's result, and `continue` on an empty row first (slots 0-2) or second (slots 3-5).
    Against the reference, and bitwise equal between two runs."""
    sc = RO.scene_C(preset, occl)
    n = sc.filt[:, 0]
    assert sc.o.shape[0] == RO.C_NRAYS > RO.C_SLOTS
    assert n[:3].tolist() == [0, 0, 0] and bool((n[1024:1027] > 0).all())
    assert bool((n[3:6] > 0).all()) and n[1027:1030].tolist() == [0, 0, 0]
    ups = sc.upstreams()
    _, g1, ref = _check("C slots", f"{preset} occl={occl}", sc, ups)
    assert float(ref.scale["mu"].min()) > 0 and float(ref.scale["opacity"].min()) > 0
    _, g2 = _launch(sc, ups, forward=False)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------
# D. upstreams
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occl", [False, True])
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("which", ["rho", "density", "trans", "all", "all-k16"])
def test_upstreams_one_at_a_time(which, preset, occl):
    """g_rho alone, g_density alone, g_trans alone (the others NULL), then all three; all-k16: 16 feature columns
    evaluated at SH degree 1.  g_trans without occlusion has no gradient: every tensor exactly zero."""
    sc = RO.scene_D(preset, occl, k16=(which == "all-k16"))
    u = sc.upstreams()
    ups = {"rho": (u[0], None, None), "density": (None, u[1], None), "trans": (None, None, u[2])}.get(which, u)
    if which == "all-k16":
        assert sc.feats.shape[1] == 16 and sc.deg == 1
    _, grads, _ = _check("D upstreams", f"{which} {preset} occl={occl}", sc, ups)
    if which == "trans" and not occl:
        assert all(bool((g == 0.0).all()) for g in grads)


@pytest.mark.parametrize("occl", [False, True])
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("s", [0, 63, 64, RO.D_NSAMP - 1])
def test_one_hot_upstream(s, preset, occl):
    """Upstreams that are zero but at one sample of every ray: the suffix scan hands sample 64's term to the
    chunk of samples 0-63 through its carry, and sample 63's along the lanes of its own chunk."""
    sc = RO.scene_D(preset, occl)
    _check("D upstreams", f"one-hot {s} {preset} occl={occl}", sc, RO.one_hot(sc, s), forward=False)


@pytest.mark.parametrize("preset", PRESETS)
def test_dead_samples_ignore_their_upstream(preset):
    """An upstream of 1e6 on every dead sample leaves all five gradient tensors bitwise equal to zeros there."""
    sc = RO.scene_D(preset, True)
    ref = sc.reference()
    assert ref.margin >= RO.MARGIN and 0.02 < float(ref.dead.float().mean()) < 0.95
    zeroed = tuple(torch.where(ref.dead, torch.zeros_like(u), u) for u in sc.upstreams())
    loud = tuple(torch.where(ref.dead, torch.full_like(u, 1e6), u) for u in zeroed)
    _, g0 = _launch(sc, zeroed, forward=False)
    _, g1 = _launch(sc, loud, forward=False)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------
# E. the largest admitted nsamp
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occl", [False, True])
@pytest.mark.parametrize("preset", PRESETS)
def test_largest_nsamp(preset, occl):
    """nsamp = 8192, what validate_rays admits: 128 chunks in the scans, (256 * 8 + 3 * 8192) * 4 B = 104 KiB of
    dynamic LDS in the backward's launch."""
    sc = RO.scene_E(preset, occl)
    assert sc.t.shape[0] == 8192
    ups = sc.upstreams()
    ref = sc.reference(ups)
    if occl:
        assert ref.first_dead() == [2000, -1]
    _check("E nsamp 8192", f"{preset} occl={occl}", sc, ups, ref)


# ---------------------------------------------------------------------------------------------------------
# F. the filter
# ---------------------------------------------------------------------------------------------------------
def _filter(o, d, bb):
    from nlosgr.rays import filter_gaussians_per_ray
    dev = _dev()
    return filter_gaussians_per_ray(o.to(dev), d.to(dev), None, bb.to(dev)).cpu()


@pytest.mark.parametrize("nrays", RO.F_NRAYS)
@pytest.mark.parametrize("ng", RO.F_NG)
def test_filter_sizes(ng, nrays):
    """Fewer boxes than a block, one more than a block, none; fewer rays than a workgroup's four and one more."""
    from oracle import torch_ref as R
    o, d, bb = RO.filter_case(ng, nrays)
    got = _filter(o, d, bb)
    ref = R.aabb_filter(o, d, bb)
    assert got.dtype == torch.int32 and got.shape == (nrays, RO.ROW)
    assert torch.equal(got, ref)
    if ng >= 63:
        assert 0 < int(ref[:, 0].sum()) < ng * nrays     # some hit, some miss
    if ng == 0:
        assert bool((got[:, 0] == 0).all()) and bool((got[:, 1:] == -1).all())


def test_filter_cap_inside_a_block():
    """400 boxes along a ray, every third (and boxes 1 to 8) moved out of its way: the 256th hit lies inside a
    block that holds more hits, so `pos < kMaxPerRay` decides; a ray that hits nothing; a ray from the far end."""
    from oracle import torch_ref as R
    o, d, bb, moved = RO.cap_midblock_boxes()
    ref = R.aabb_filter(o, d, bb)
    hits = torch.nonzero(~moved).flatten()
    last = int(hits[255])
    assert last % 64 < 60 and int(((hits > last) & (hits // 64 == last // 64)).sum()) > 0
    assert ref[:, 0].tolist() == [256, 0, 256] and int(ref[0, 256]) == last
    assert torch.equal(ref[0, 1:], hits[:256].int())
    got = _filter(o, d, bb)
    assert torch.equal(got, ref)


def test_filter_special_rays():
    """Directions with a component exactly 0 (1 / (0 + 1e-8)) and negative components, an origin inside a box, a
    box wholly behind the origin, a ray that hits nothing (rays_oracle.special_rays; test_rays_oracle_cpu.py pins
    which ray hits what)."""
    from oracle import torch_ref as R
    o, d, bb, want = RO.special_rays()
    ref = R.aabb_filter(o, d, bb)
    for r, idx in enumerate(want):
        assert ref[r, :1 + len(idx)].tolist() == [len(idx)] + idx
    assert torch.equal(_filter(o, d, bb), ref)


# ---------------------------------------------------------------------------------------------------------
# G. empty sizes and invalid arguments through the C ABI
# ---------------------------------------------------------------------------------------------------------
def _abi(ng, nrays, nsamp, k_feat=1, deg=0):
    """(lib, Gaussians, Rays, tensors) with every array allocated (at least one element, so no pointer is NULL)."""
    from nlosgr import _lib
    lib, dev = _lib.load(), _dev()
    z = lambda *s: torch.zeros(*[max(x, 1) for x in s], device=dev)
    T = dict(mu=z(ng, 3), sc=z(ng, 3), rot=z(ng, 4), op=z(ng), ft=z(ng, k_feat), o=z(nrays, 3), d=z(nrays, 3),
             t=z(nsamp), cam=z(3))
    T["rot"][:, 0] = 1.0
    T["d"][:, 1] = 1.0
    p = _lib.ptr
    g = _lib.Gaussians(ng, k_feat, deg, _lib.PRESET_CUDA, 1.0, p(T["mu"]), p(T["sc"]), p(T["rot"]), p(T["op"]),
                       p(T["ft"]))
    r = _lib.Rays(nrays, nsamp, p(T["o"]), p(T["d"]), p(T["t"]), p(T["cam"]))
    return lib, g, r, T


@pytest.mark.parametrize("occl", [0, 1])
def test_abi_no_gaussians(occl):
    """ng = 0: the forward gives 0, 0 and 1 everywhere (no workspace needed), the backward returns OK."""
    from nlosgr import _lib
    lib, g, r, T = _abi(0, 5, 70)
    dev = _dev()
    filt = RO.rows([[]] * 5).to(dev)
    out = [torch.full((5, 70), 7.0, device=dev) for _ in range(3)]
    rc = lib.nlosgr_rays_fwd(g, r, _lib.ptr(filt), 0.3, occl, None, *[_lib.ptr(x) for x in out], _lib.stream_handle(dev))
    assert rc == 0, lib.nlosgr_last_error()
    assert bool((out[0] == 0.0).all()) and bool((out[1] == 0.0).all()) and bool((out[2] == 1.0).all())
    rc = lib.nlosgr_rays_bwd(g, r, _lib.ptr(filt), 0.3, occl, None, _lib.ptr(out[0]), None, None, None, None, None, None,
                             None, _lib.stream_handle(dev))
    assert rc == 0, lib.nlosgr_last_error()


@pytest.mark.parametrize("occl", [0, 1])
def test_abi_no_rays(occl):
    """nrays = 0: the backward gives all-zero gradients (the outputs are overwritten, whatever they held); no ray
    means no filter row and no upstream, so those pointers are NULL, as an empty tensor's is."""
    from nlosgr import _lib
    lib, g, r, T = _abi(9, 0, 70, k_feat=4, deg=1)
    dev = _dev()
    assert torch.empty(0, RO.ROW, dtype=torch.int32, device=dev).data_ptr() == 0
    ws = torch.empty(max(lib.nlosgr_rays_workspace_bytes(g, r), 1), dtype=torch.uint8, device=dev)
    outs = [torch.full(s, 7.0, device=dev) for s in ((9, 3), (9, 3), (9, 4), (9,), (9, 4))]
    rc = lib.nlosgr_rays_bwd(g, r, None, 0.3, occl, _lib.ptr(ws), None, None, None, *[_lib.ptr(x) for x in outs],
                             _lib.stream_handle(dev))
    assert rc == 0, lib.nlosgr_last_error()
    for x in outs:
        assert bool((x == 0.0).all())


def test_abi_rejects():
    """nsamp = 8193 is NLOSGR_E_UNSUPPORTED (8192 is admitted: test_largest_nsamp), k_feat < (deg + 1)^2 is
    NLOSGR_E_INVALID, each with a message."""
    E_INVALID, E_UNSUPPORTED = 1, 3
    for (nsamp, k_feat, deg), want in (((8193, 1, 0), E_UNSUPPORTED), ((70, 3, 1), E_INVALID), ((70, 15, 3), E_INVALID)):
        from nlosgr import _lib
        lib, g, r, T = _abi(4, 2, nsamp, k_feat, deg)
        dev = _dev()
        filt = RO.rows([[0, 1], [2]]).to(dev)
        out = [torch.zeros(2, nsamp, device=dev) for _ in range(3)]
        ws = torch.empty(4096, dtype=torch.uint8, device=dev)
        assert lib.nlosgr_rays_workspace_bytes(g, r) == 0
        rc = lib.nlosgr_rays_fwd(g, r, _lib.ptr(filt), 0.3, 0, _lib.ptr(ws), *[_lib.ptr(x) for x in out],
                                 _lib.stream_handle(dev))
        assert rc == want and len(lib.nlosgr_last_error()) > 0
        gr = [torch.zeros(s, device=dev) for s in ((4, 3), (4, 3), (4, 4), (4,), (4, k_feat))]
        rc = lib.nlosgr_rays_bwd(g, r, _lib.ptr(filt), 0.3, 0, _lib.ptr(ws), _lib.ptr(out[0]), None, None,
                                 *[_lib.ptr(x) for x in gr], _lib.stream_handle(dev))
        assert rc == want and len(lib.nlosgr_last_error()) > 0
