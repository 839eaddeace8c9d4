"""The SGLD noise step without a GPU: the generator (tests/sgld_oracle.py and csrc/nlosgr_rng.hpp through a
stand-alone host program) against the Random123 known answers, the pinned normals that fix the counter layout and
the Box-Muller pairing, the statistics of the oracle's noise, and the Python side: the new OptimizationParams
fields, densify.mcmc_control's schedule and the new command-line flags.

Statistics: the bounds are 5 standard errors of each estimator at N = 65536 (mean and covariance 1 / sqrt(N), variance
sqrt(2 / N)); the oracle stays within 2.6 on every case.
"""
import math
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

import sgld_oracle as SO

CSRC = os.path.join(ROOT, "nlos-gaussian-renderer_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "sgld_rng_main.cpp")

# Random123's known answers for philox4x32-10: (counter, key, output)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
CASES = [(0, 0), (0, 1), (1234, 7), (2 ** 40 + 5, 2 ** 33 + 1)]    # (seed, iteration); the last needs the high words
N = 65536


def test_oracle_philox_known_answers():
    for c, k, want in KAT:
        got = SO.philox4x32_10(np.array(c, dtype=np.uint64), np.array(k, dtype=np.uint64))
        assert tuple(int(v) for v in got) == want
    # the library's binding and Python entry points exist (they do not on a tree without the feature)
    from nlosgr import _lib, densify, train
    assert "nlosgr_sgld_noise" in _lib.EXPORTS and hasattr(_lib.load(), "nlosgr_sgld_noise")
    assert callable(train.sgld_noise) and callable(densify.mcmc_control)


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def test_host_program_matches_known_answers_and_oracle(tmp_path):
    """csrc/nlosgr_rng.hpp, the very header the kernel includes, compiled for the host with the address and
    undefined-behaviour sanitizers: the three known answers, and words and uniforms equal to the oracle's, bit for
    bit (the uniforms are printed with nine digits, which round-trips fp32)."""
    exe = str(tmp_path / "sgld_rng")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, MAIN, "-o", exe]
    hipcc = _hipcc()
    if hipcc:
        cmd = [hipcc, "-x", "hip", "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
               "-fno-sanitize-recover=all"] + flags
    else:
        cxx = shutil.which("g++") or shutil.which("clang++")
        assert cxx, "a host C++ compiler is needed"
        cmd = [cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + flags
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    kats = [ln.split() for ln in lines if ln.startswith("kat ")]
    assert len(kats) == 3
    for (c, k, want), f in zip(KAT, kats):
        assert tuple(int(v, 16) for v in f[1:7]) == c + k
        assert tuple(int(v, 16) for v in f[8:12]) == want
    draws = [ln.split() for ln in lines if ln.startswith("draw ")]
    assert len(draws) >= 6
    for f in draws:
        seed, it, n = int(f[1]), int(f[2]), int(f[3])
        w = SO.words(seed, it, np.array([n], dtype=np.uint64))[0]
        assert [int(v, 16) for v in f[5:9]] == [int(v) for v in w], f
        u = SO.uniforms(w)
        assert [np.float32(v) for v in f[10:14]] == [np.float32(v) for v in u], f
        assert all(float(np.float32(v)) == float(v) for v in u)        # exact in fp32
    ends = [ln.split() for ln in lines if ln.startswith("ends ")][0]
    assert np.float32(ends[1]) == np.float32(2.0 ** -24) and np.float32(ends[2]) == np.float32(1.0 - 2.0 ** -24)


def test_pinned_normals():
    """(seed, iteration) = (42, 5), n = 0, 1, 2: pins the counter layout and the Box-Muller pairing."""
    want = np.array([[-1.0155149, 0.6529852, 0.8418711], [0.1639463, -1.0049414, -1.4030355],
                     [1.7261147, -0.3336660, -0.1154606]])
    got = SO.xi_of(42, 5, np.arange(3, dtype=np.uint64))
    assert np.abs(got - want).max() <= 1e-6, got


def _noise(seed, it):
    """The oracle's delta for N unit-covariance Gaussians with gate = 1/2 (gate_k = 0) and scale = 2: xi itself up to
    the cuda preset's (1 + 1e-8)^2."""
    S = np.zeros((N, 3), dtype=np.float32)
    Q = np.zeros((N, 4), dtype=np.float32)
    Q[:, 0] = 1.0
    ref = SO.reference(S, Q, np.zeros(N, dtype=np.float32), "cuda", 1.0, seed, it, 0, 2.0, gate_k=0.0)
    assert np.abs(ref["delta"] - ref["xi"]).max() <= 1e-7 * np.abs(ref["xi"]).max()
    return ref["delta"]


@pytest.mark.parametrize("seed,it", CASES)
def test_oracle_noise_statistics(seed, it):
    x = _noise(seed, it)
    se = 1.0 / math.sqrt(N)
    mean = x.mean(0)
    var = x.var(0)
    cov = np.cov(x.T, bias=True)
    y = _noise(seed, it + 1)                                    # the next iteration's noise
    cross = np.array([np.corrcoef(x[:, c], y[:, d])[0, 1] for c in range(3) for d in range(3)])
    off = np.abs(cov[np.triu_indices(3, 1)])
    print(f"\n(seed, it) = ({seed}, {it}): |mean| {np.abs(mean).max() / se:.2f} se, |var - 1| "
          f"{np.abs(var - 1).max() / (math.sqrt(2) * se):.2f} se, |cov| {off.max() / se:.2f} se, "
          f"|corr(it, it + 1)| {np.abs(cross).max() / se:.2f} se")
    assert np.abs(mean).max() <= 5 * se
    assert np.abs(var - 1).max() <= 5 * math.sqrt(2.0 / N)
    assert off.max() <= 5 * se
    assert np.abs(cross).max() <= 5 * se


def test_iterations_zero_and_one_are_uncorrelated():
    x, y = _noise(0, 0), _noise(0, 1)
    assert max(abs(np.corrcoef(x[:, c], y[:, c])[0, 1]) for c in range(3)) <= 5 / math.sqrt(N)


def test_high_words_of_seed_and_iteration_count():
    n = np.arange(64, dtype=np.uint64)
    full = SO.xi_of(2 ** 40 + 5, 2 ** 33 + 1, n)
    assert not np.array_equal(full, SO.xi_of(5, 1, n))                       # both truncated to 32 bits
    assert not np.array_equal(full, SO.xi_of(5, 2 ** 33 + 1, n))             # the seed alone
    assert not np.array_equal(full, SO.xi_of(2 ** 40 + 5, 1, n))             # the iteration alone
    hi = SO.xi_of(42, 5, n + np.uint64(2 ** 32))                             # and the index's high word
    assert not np.array_equal(hi, SO.xi_of(42, 5, n))


def test_library_validates_without_a_gpu():
    """Null pointers, ng < 0 and an unknown preset are NLOSGR_E_INVALID before any launch; ng == 0 is valid."""
    import ctypes
    from nlosgr import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    o = _lib.Sgld(1, 2, 3, 1.0, 100.0, 0.995)
    assert ctypes.sizeof(_lib.Sgld) == 40
    ok = _lib.Gaussians(4, 0, 0, _lib.PRESET_CUDA, 1.0, fake, fake, fake, fake, None)
    call = lambda g, o, out: lib.nlosgr_sgld_noise(ctypes.byref(g) if g else None, ctypes.byref(o) if o else None, out,
                                                   None, None)
    assert call(None, o, fake) == 1 and call(ok, None, fake) == 1
    assert call(ok, o, None) == 1 and b"mu_out" in lib.nlosgr_last_error()
    for k in range(4):                                   # a null mu, scaling, rotation, opacity
        ptrs = [fake] * 4
        ptrs[k] = None
        assert call(_lib.Gaussians(4, 0, 0, _lib.PRESET_CUDA, 1.0, *ptrs, None), o, fake) == 1
    assert call(_lib.Gaussians(-1, 0, 0, _lib.PRESET_CUDA, 1.0, fake, fake, fake, fake, None), o, fake) == 1
    assert call(_lib.Gaussians(4, 0, 0, 7, 1.0, fake, fake, fake, fake, None), o, fake) == 1
    assert b"preset" in lib.nlosgr_last_error()
    assert call(_lib.Gaussians(0, 0, 0, _lib.PRESET_TORCH, 1.0, None, None, None, None, None), o, None) == 0


def test_noise_is_off_by_default():
    from nlosgr.train import OptimizationParams
    o = OptimizationParams()
    assert o.noise_lr == 0 and o.noise_seed == 0 and o.noise_gate_k == 100.0 and o.noise_gate_x0 == 0.995


class _StubStep:
    """What densify takes from a train step on the CPU: the model, the iteration, the Adam moments and rebind."""

    def __init__(self, model):
        self.model, self.iteration, self.rebinds = model, 0, 0
        self._bind()

    def _bind(self):
        m = self.model
        shapes = [getattr(m, n).shape for n in ("_mu", "_features_dc", "_features_rest", "_opacity", "_scaling",
                                                "_rotation")]
        self.adam = SimpleNamespace(exp_avg=[torch.ones(s) for s in shapes], exp_avg_sq=[torch.ones(s) for s in shapes])

    def rebind(self, exp_avg=None, exp_avg_sq=None):
        self.rebinds += 1
        self._bind()
        for i, (a, b) in enumerate(zip(exp_avg, exp_avg_sq)):
            self.adam.exp_avg[i].copy_(a)
            self.adam.exp_avg_sq[i].copy_(b)


def _schedule_fires(it, from_iter, until_iter, interval):
    return it < until_iter and it > from_iter and it % interval == 0       # main.py:244, on the finished-step count


def test_mcmc_control_fires_on_the_reference_schedule():
    from nlosgr import GaussianParams
    from nlosgr.densify import mcmc_control
    torch.manual_seed(0)
    m = GaussianParams.synthetic(40, 1, preset="cuda", device="cpu", seed=2)
    step = _StubStep(m)
    fired = []
    for it in range(0, 40):
        step.iteration = it
        before = m._mu.shape[0]
        got = mcmc_control(step, from_iter=10, until_iter=30, interval=5, cap_max=10 ** 6)
        if got is not None:
            fired.append(it)
            assert got == int(1.05 * before) - before and m._mu.shape[0] == before + got
        else:
            assert m._mu.shape[0] == before
        assert (got is not None) == _schedule_fires(it, 10, 30, 5)
    assert fired == [15, 20, 25]                       # strictly between from and until
    assert step.rebinds == 3
    assert mcmc_control(_StubStep(m)) is None          # iteration 0 under the defaults


def test_mcmc_control_relocates_grows_and_stops_at_the_cap():
    from nlosgr import GaussianParams
    from nlosgr.densify import mcmc_control, prune_dead_mask
    torch.manual_seed(1)
    m = GaussianParams.synthetic(100, 1, preset="cuda", device="cpu", seed=3)
    m._opacity.data[:7] = -12.0                        # dead
    m._opacity.data[7:] = m._opacity.data[7:].clamp_min(-2.0)
    live_mu = m._mu.data[7:].clone()
    step = _StubStep(m)
    step.iteration = 600
    assert mcmc_control(step, cap_max=103) == 3        # 5 % would be 5: the cap holds it at 103
    assert m._mu.shape[0] == 103 and m._scaling.shape[0] == 103 and m._features_rest.shape[0] == 103
    assert int(prune_dead_mask(m).sum()) == 0
    d = (m._mu.data[:7, None, :] - live_mu[None]).abs().amax(-1).amin(1)
    assert (d == 0).all()                              # the dead were moved onto live ones (relocate_gs)
    assert step.adam.exp_avg[0].shape == (103, 3) and bool((step.adam.exp_avg[0][100:] == 0).all())
    assert bool((step.adam.exp_avg[0] == 0).any(dim=1)[:100].any())          # sampled sources' moments were reset
    step.iteration = 700
    assert mcmc_control(step, cap_max=103) == 0 and m._mu.shape[0] == 103     # at the cap: fires, adds nothing
    step.iteration = 800
    assert mcmc_control(step, cap_max=200) == 5 and m._mu.shape[0] == 108


# the fields and defaults of the two command lines before the new flags (recorded from their parsers)
_NC_BEFORE = dict(capture="c.mat", start=3, end=9, ns=32, gaussians=5, iterations=2, cutoff=5.7, resolution=64,
                  loss="mse", out="o.pth")
_VF_BEFORE = dict(capture="c.mat", resolution=64, start=3, end=9, gaussians=5, iterations=2, power=0, falloff=0.0,
                  cutoff=3.0, loss="mse", out="o.pth", recon=None)
_NEW_DEFAULTS = dict(noise_lr=0.0, noise_seed=0, densify_interval=0, densify_from=500, densify_until=25_000,
                     cap_max=100_000)
_ARGV = ["c.mat", "--start", "3", "--end", "9", "--gaussians", "5", "--iterations", "2", "--out", "o.pth"]


@pytest.mark.parametrize("module,before", [("render_nc", _NC_BEFORE), ("voxel_fit", _VF_BEFORE)])
def test_command_line_flags(module, before):
    import importlib
    from nlosgr.train import OptimizationParams, mcmc_options
    mod = importlib.import_module("nlosgr." + module)
    a = vars(mod.parse_args(_ARGV))
    assert a == {**before, **_NEW_DEFAULTS}
    assert mcmc_options(SimpleNamespace(**a)) is None               # the step's own default options: today's run
    b = mod.parse_args(_ARGV + ["--noise-lr", "5e5", "--noise-seed", "7", "--densify-interval", "100", "--densify-from",
                                "50", "--densify-until", "900", "--cap-max", "4000"])
    assert (b.noise_lr, b.noise_seed, b.densify_interval, b.densify_from, b.densify_until, b.cap_max) == \
        (5e5, 7, 100, 50, 900, 4000)
    assert {k: v for k, v in vars(b).items() if k in before} == before
    assert mcmc_options(b) == OptimizationParams(noise_lr=5e5, noise_seed=7)
    for bad in (["--noise-lr", "-1"], ["--densify-interval", "-3"], ["--cap-max", "0"]):
        with pytest.raises(SystemExit):
            mod.parse_args(_ARGV + bad)
