"""The twin drain's loop, replayed on the CPU (scripts/refill_replay.py), must end on every shape of
tests/test_gpu_fx_refill.py and take exactly the queue entries it enumerated (plus the split twins it re-queued):
a wrong refill rule is a hang on the GPU, so it is tried here first.  Each shape runs under the tail rule with
the kernel's diagnostics flags 0, 1 (entries taken, never set up) and 4 (no lane ever active), and under the
parent rule; a replay that does not end raises refill_replay.Hang.  One wall point per shape keeps it quick.
"""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

CUT = 5.7


def _load():
    spec = importlib.util.spec_from_file_location("refill_replay", os.path.join(ROOT, "scripts", "refill_replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RR = _load()


def _scene(T=256, ns=16, **kw):
    from nlosgr.volume import Scene
    return Scene(H=3, W=3, T=T, ns=ns, **kw)


def _arrays(ng, edit=None):
    from nlosgr import GaussianParams
    m = GaussianParams.synthetic(max(ng, 1), 3, preset="cuda", device=torch.device("cpu"), seed=21)
    with torch.no_grad():
        if edit is not None:
            edit(m)
    return tuple(t.detach()[:ng].double().numpy() for t in (m._mu, m._scaling, m._rotation))


def _identical(ng):
    mu = np.tile(np.array([[0.0, 0.5, 0.0]]), (ng, 1))
    sc = np.full((ng, 3), math.log(0.06))
    rot = np.tile(np.array([[0.3, -0.5, 0.7, 0.1]]), (ng, 1))
    return mu, sc, rot


def _thin(m):
    m._scaling[:, 1] = math.log(3e-4)


SHAPES = {
    "1500": (lambda: _arrays(1500), {}),
    "2600": (lambda: _arrays(2600), {}),
    "70": (lambda: _arrays(70), {}),
    "1": (lambda: _arrays(1), {}),
    "0": (lambda: _arrays(0), {}),
    "64 identical": (lambda: _identical(64), {}),
    "thin": (lambda: _arrays(1500, _thin), {}),
    "ns 5": (lambda: _arrays(1500), {"ns": 5}),
    "T 41": (lambda: _arrays(1500), {"T": 41, "start": 90, "deltaT": 5e-3}),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_replay_ends_and_takes_every_entry(name):
    make, skw = SHAPES[name]
    mu, sc, rot = make()
    geo = _scene(**skw).geometry(torch.device("cpu"), "cuda", "noocl")
    got = {}
    for rule, flags in (("tail", 0), ("tail", 1), ("tail", 4), ("parent", 0)):
        if len(mu) == 0:
            # no pairs: every wave runs the final pass alone
            c = RR.replay_wave(None, [], rule=rule, flags=flags)
        else:
            c = RR.replay_scene(geo, mu, sc, rot, cutoff=CUT, walls=[4], rule=rule, flags=flags, limit=2_000_000)
        got[(rule, flags)] = c
        assert c["entries_taken"] == c["enumerated"] + c["requeued"], (name, rule, flags, c)
        if flags:
            assert c["rounds"] == 0, (name, rule, flags, c)
    t, p = got[("tail", 0)], got[("parent", 0)]
    print(f"\n{name}: tail rule rounds {t['rounds']} refills {t['refills']} (< 32: {t['refills_under_32']}); parent "
          f"rule rounds {p['rounds']} refills {p['refills']} (< 32: {p['refills_under_32']}); re-queued {t['requeued']}")
    assert t["entries_taken"] == p["entries_taken"]   # the rules drain the same entries
    if name not in ("0",):
        assert t["enumerated"] > 0 and t["rounds"] > 0
    if name == "thin":
        assert t["requeued"] > 0, "no twin was split: the re-queue in the tail was not replayed"
    if name == "2600":
        assert RR.fwd_nsplit(2600, geo.nwall) == 8 and len(RR.wave_chunks(2600, 8, 0, 0)) == 2
