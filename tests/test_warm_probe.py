"""The warm start's probe (hdsm_wave_gib.h, WaveGIB::warm_start) in the CPU execution of the device source: a guessed row is tested
for the multiplier it would get before it is installed, and left out if that multiplier is negative.

tests/golden/warm_probe_ring.npz (tests/golden/make_warm_probe_golden.py) holds recorded rounds of a ring of 16 agents at 1 m
chord: H = 10 for the NV = 32 kernels and H = 12 for the NV = 48 kernels (a shape refuses an n of the other layout). They are
replayed with the warm store carried over, in both wave orders, on the shapes `quad` and `duo48`, and compared with the
oracle, which is cold-started on every round. The counts of what the warm start did come from a second build of the CPU
execution (tests/warm_probe_emu) that defines the hooks of hdsm_wave_gib.h; that build also forms the multiplier of every accepted
row the long way (t = U^T v, lambda = U t on the set as it stands) next to the probe's.

NV = 48 keeps the install-everything order (it has no registers for the probe): its replays check that the answers stay the
oracle's, and that no guessed row is rejected there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import problems
from multi_agent_pkgs_amd.params import agile_params, make_params
from warm_probe_cases import HERE, KEYS, REPLAYS, compare, ring, ring_oracle  # noqa: F401  (fixtures: one oracle pass for the module)

EVENTS = ("reject", "accept", "drop_new", "drop_old", "box_row")   # hdsm::WarmEvent
@pytest.fixture(scope="module")
def wave():
    from wave_emu import pywave
    pywave.lib()
    return pywave


class Audit:
    """The CPU execution built with the warm-start hooks; replan() is pywave.replan on that library."""

    def __init__(self, pywave):
        d = os.path.join(HERE, "warm_probe_emu")
        subprocess.check_call(["make", "-C", d, "-s"])
        self.lib = C.CDLL(os.path.join(d, "libhdsm_warm_probe_emu.so"))
        self.lib.wave_last_error.restype = C.c_char_p
        self.pywave = pywave

    def replan(self, *args, **kw):
        keep = self.pywave._lib
        self.pywave._lib = self.lib
        try:
            return self.pywave.replan(*args, **kw)
        finally:
            self.pywave._lib = keep

    def counts(self):
        """Events since the last call, the accepted rows checked and their largest relative multiplier difference."""
        n = len(EVENTS)
        out = (C.c_long * (n + 1))()
        worst = C.c_double()
        assert self.lib.wave_warm_audit(out, C.byref(worst), 1) == n
        d = {k: int(out[i]) for i, k in enumerate(EVENTS)}
        d["checked"], d["worst"] = int(out[n]), float(worst.value)
        return d


@pytest.fixture(scope="module")
def audit(wave):
    return Audit(wave)


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("name,horizon,shape", REPLAYS, ids=[r[2] for r in REPLAYS])
def test_ring_replay_matches_the_oracle(wave, ring, ring_oracle, monkeypatch, name, horizon, shape, order):
    """The product's source as the GPU runs it, warm store carried over."""
    if order == "reverse":
        monkeypatch.setenv("WEMU_ORDER", "reverse")
    prm = agile_params(horizon, max_rows_static=18)
    store = wave.new_warm_store(16)
    warm_rounds = 0
    for r, o in zip(ring[name], ring_oracle[name]):
        warm_rounds += int(((store[:, 0] & 0xffff) > 0).any())
        compare(wave.replan(prm, *[r[k] for k in KEYS], warm=store, shape=shape), o)
    assert warm_rounds >= len(ring[name]) - 2     # the store does seed the rounds after the first


def test_ring_recording_holds_what_it_is_for(audit, ring, ring_oracle):
    """The audit build on the same replays. H = 10 (NV = 32): at least one guessed row is rejected by the probe, at least one
    accepted row is dropped by the fix-up afterwards, at least one guess holds a row of an input or state box; every accepted
    row's multiplier from the probe equals the one of the full evaluation on the same set. H = 12 (NV = 48): rows are installed
    and dropped, none is rejected."""
    seen = {}
    for name, horizon, shape in REPLAYS:
        prm = agile_params(horizon, max_rows_static=18)
        store = audit.pywave.new_warm_store(16)
        audit.counts()
        for r, o in zip(ring[name], ring_oracle[name]):
            compare(audit.replan(prm, *[r[k] for k in KEYS], warm=store, shape=shape), o)
        seen[name] = audit.counts()
        print(name, seen[name])
    a = seen["h10"]
    assert a["reject"] >= 1 and a["drop_new"] >= 1 and a["box_row"] >= 1 and a["accept"] >= 1, a
    # probe and full evaluation are the same triangular solve in a different order of operations: rounding only, amplified by the
    # condition of R (rows of a squeezed ring are nearly parallel) — eight digits is what the suite asks of the answers themselves
    assert a["checked"] == a["accept"] and a["worst"] < 1e-8, a
    b = seen["h12"]
    assert b["reject"] == 0 and b["checked"] == 0, b


def test_a_store_written_before_the_probe_is_accepted(audit, wave, ring, ring_oracle):
    """The fixture holds the warm store the build of the commit BEFORE the probe left after h10's first two rounds (the handle's record
    format: count | certificate bit, then portable ids). This build writes the same records for the same rounds, and continues
    from the old build's store: its rows are installed (and probed), every later round gives the oracle's answer."""
    done, old = ring["parent_store"]
    assert old.dtype == np.int32 and old.shape == (16, wave.MAXNV + 2) and ((old[:, 0] & 0xffff) > 0).all()
    prm = agile_params(10, max_rows_static=18)
    own = wave.new_warm_store(16)
    for r in ring["h10"][:done]:
        wave.replan(prm, *[r[k] for k in KEYS], warm=own, shape="quad")
    # same heads (row counts, certificate bits) and the same sets of ids, whatever path led to them: the optimum's working set
    assert np.array_equal(own[:, 0], old[:, 0]), (own[:, 0].tolist(), old[:, 0].tolist())
    for a in range(16):
        cnt = int(old[a, 0] & 0xffff)
        assert sorted(own[a, 1:1 + cnt].tolist()) == sorted(old[a, 1:1 + cnt].tolist()), a
    store = old.copy()
    audit.counts()
    first = True
    for r, o in zip(ring["h10"][done:], ring_oracle["h10"][done:]):
        compare(audit.replan(prm, *[r[k] for k in KEYS], warm=store, shape="quad"), o)
        if first:
            c = audit.counts()
            print(c)
            assert c["accept"] >= 1 and c["reject"] >= 1 and c["checked"] == c["accept"] and c["worst"] < 1e-8, c
            first = False
    store = old.copy()
    for r, o in zip(ring["h10"][done:], ring_oracle["h10"][done:]):
        compare(wave.replan(prm, *[r[k] for k in KEYS], warm=store, shape="quad"), o)


def test_crafted_guess_with_a_row_that_must_go(audit, wave, oracle):
    """Three agents, H = 7, all with a solution. The first replan fills the store; its working sets hold rows of the input boxes
    (the agents brake or push at the jerk limit) next to neighbour planes. Then every reference is mirrored through the agent's
    position: the unconstrained minimiser now pulls the other way, the box rows of the guess lie on the far side of it and would
    enter with a negative multiplier. The probe must leave such rows out, and the answers stay the oracle's."""
    prm = make_params(n_hor=7, max_rows_static=18)
    sn = problems.swarm_snapshot(prm, 3, seed=3, spacing=1.2)
    args = [sn[k] for k in KEYS]
    store = wave.new_warm_store(3)
    o1 = oracle.replan(prm, *args, n_threads=8)
    assert (o1["status"] == 0).all()
    compare(audit.replan(prm, *args, warm=store), o1)
    assert (((store[:, 0] & 0xffff) > 0) & (store[:, 0] < (1 << 30))).all()   # three working sets to start from
    stale = store.copy()
    audit.counts()
    turned = dict(sn)
    turned["ref"] = sn["ref"].copy()
    turned["ref"][:, :, :3] = 2.0 * sn["state"][:, None, :3] - sn["ref"][:, :, :3]
    turned["ref"][:, :, 3:] = -sn["ref"][:, :, 3:]
    args2 = [turned[k] for k in KEYS]
    o2 = oracle.replan(prm, *args2, n_threads=8)
    compare(audit.replan(prm, *args2, warm=store), o2)
    c = audit.counts()
    print(c)
    assert c["reject"] >= 1 and c["box_row"] >= 1 and c["checked"] == c["accept"] and c["worst"] < 1e-8, c
    compare(wave.replan(prm, *args2, warm=stale), o2)    # ... and the build without the audit, from the same stale store
