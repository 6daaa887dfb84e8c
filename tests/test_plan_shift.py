"""The cases of tests/shift_cases.py, judged from the oracle alone on the CPU, so that tests/test_gpu_plan_shift.py cannot pass on
a library that ignores a shift or the own-plan override:

  * in at least half the instances of every case the oracle's answer for the shifted view differs from its answer for the
    unshifted view by more than 1e-3 m;
  * in the override batch the answer with the decoy taken as the own record differs from the right one by more than 1e-3 m, in at
    least half the instances too;
  * the reference row (path_vel) and the planes differ between the two views as well;
  * the sphere case: what the issue asked for — a neighbour whose UNSHIFTED sphere is culled and whose shifted positions give an
    active plane — cannot exist, and the test below states why and what is checked instead."""
import numpy as np
import pytest

import shift_cases as sc


@pytest.mark.parametrize("idx", range(len(sc.CASES)), ids=sc.IDS)
def test_the_cases_can_see_an_ignored_shift_and_an_ignored_override(oracle, idx):
    c = sc.case(idx)
    N = c.n_hor
    assert set(c.shift[:5].tolist()) == {0, 1, N - 1, N, N + 3} and (c.shift % c.step_plan == 0)[5:10].all() and (c.shift == 0).sum() == 1
    shifted, plain = c.want(oracle, "shifted"), c.want(oracle, "unshifted")
    d = sc.moved(shifted, plain)
    print(f"{sc.IDS[idx]}: shifted against unshifted view, instances moved > 1e-3 m: {int((d > 1e-3).sum())} of {sc.N_ROB}, median {np.median(d):.3f} m;"
          f" no solution {int((shifted['status'] == 2).sum())} / {int((plain['status'] == 2).sum())}")
    assert (d > 1e-3).sum() >= sc.N_ROB // 2
    assert (shifted["status"] != 2).sum() >= sc.N_ROB // 2          # ... and most of what is compared is a trajectory
    right, wrong = c.want(oracle, "override"), c.want(oracle, "decoy")
    d = sc.moved(right, wrong)
    print(f"{sc.IDS[idx]}: override against decoy as own record, moved > 1e-3 m: {int((d > 1e-3).sum())} of {sc.N_ROB}, median {np.median(d):.3f} m")
    assert (d > 1e-3).sum() >= sc.N_ROB // 2
    assert (right["status"] != 2).sum() >= sc.N_ROB // 2
    # agent 5 flies its own plan although nobody sees it: its answer needs own_has, not has_plan
    assert c.decoy_has[5] == 0 and c.own_has[5] == 1


@pytest.mark.parametrize("idx", [1, 5], ids=[sc.IDS[1], sc.IDS[5]])
def test_the_reference_row_and_the_planes_see_the_shift_too(oracle, idx):
    c = sc.case(idx)
    sn = c.sn
    for monotone in (True, False):
        _, _, pv = c.want_reference(oracle, monotone, override=False)
        _, _, pv0 = oracle.reference(c.prm(), c.ref_cfg(monotone), sn["agent_id"], c.path, c.n_path, sn["plans"], sn["has_plan"])
        # (a path velocity is set by the ONE closest (neighbour, step) pair: a quarter of the instances is asked for, not half)
        assert (np.abs(pv - pv0) > 1e-3).sum() >= sc.N_ROB // 4, (monotone, pv, pv0)
    a = 0
    m, h = sc.view_of(a, sn["plans"], sn["has_plan"], c.shift)
    p1, _ = oracle.tasc_planes(c.prm(), a, sn["state"][a], m, h)
    p0, _ = oracle.tasc_planes(c.prm(), a, sn["state"][a], sn["plans"], sn["has_plan"])
    assert np.abs(p1 - p0).max() > 1e-3


def test_materialise_is_the_definition():
    rng = np.random.default_rng(1)
    plans = rng.normal(size=(4, 8, 9))
    m = sc.materialise(plans, [0, 3, 7, 12])
    assert (m[0] == plans[0]).all() and (m[1, :5] == plans[1, 3:]).all() and (m[1, 5:] == plans[1, 7]).all()
    assert (m[2] == plans[2, 7]).all() and (m[3] == plans[3, 7]).all()


def test_a_shifted_record_is_a_subset_of_the_record_so_its_sphere_only_shrinks():
    """The issue asks for a prefilter case with a neighbour whose unshifted sphere is culled and whose shifted positions give an
    active plane. No such neighbour exists: the shifted positions R[min(i + s, N)], i = 1..N, are a SUBSET of the unshifted ones
    R[1..N]; the sphere that holds the unshifted positions holds the shifted ones, and the cull is rigorous for every point inside
    the sphere (hdsm_wave_gi.h, sweep_planes). What CAN go wrong is the other direction, and it is what sphere_case holds: a
    neighbour whose unshifted sphere reaches every agent while its shifted positions are one point far from most of them. With
    bounds left unshifted the answers stay right and the prefilter stops culling; with `pos` left unshifted and bounds shifted, the
    sweeps would skip a neighbour whose (unshifted) positions matter. tests/test_gpu_plan_shift.py checks both through the answers
    and the sweep statistics. Here: the geometry of the case."""
    prm, sn, shift = sc.sphere_case()
    pos, shifted = sn["plans"][8, 1:, :3], sc.materialise(sn["plans"], shift)[8, 1:, :3]
    assert all(any((p == q).all() for q in pos) for p in shifted)                      # a subset
    c0, c1 = 0.5 * (pos.min(0) + pos.max(0)), 0.5 * (shifted.min(0) + shifted.max(0))
    r0, r1 = np.linalg.norm(pos - c0, axis=1).max(), np.linalg.norm(shifted - c1, axis=1).max()
    assert r1 == 0.0 and r0 > 20.0
    own = sn["plans"][:8, 1, :3]
    assert (np.linalg.norm(own - c0, axis=1) < r0 + 5.0).all()                         # unshifted: inside everybody's reach
    far = np.linalg.norm(own - c1, axis=1)
    assert far[0] < 1.3 and (far[4:] > 4.5).all()                                      # shifted: beside agent 0, metres from agents 4..7
