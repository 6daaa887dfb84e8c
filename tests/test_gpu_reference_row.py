"""Row f1 on the MI355X where no other test reaches it: hdsm_reference (and hdsm_reference_device where named) against the
oracle's orc_reference on the cases of tests/reference_cases.py — the survivor list drained in mid-scan in both launch forms,
shuffled subsets of a larger swarm, id ranges that start above 0, polylines read from global memory, counts only the device entry
clamps, non-finite plans, the pairwise branch. tests/test_reference_row.py pins the oracle on the same cases to a long-double
rendering and asserts that the cases can see a failure.

Tolerance: the row's own, 1e-10 * max(1, |y|.max()) per output (tests/test_gpu_parity.py::test_reference_kernel_matches_oracle).
Every case is called twice on one handle, with the case's vel_cap and with the other choice (none / a drawn one): the second call
packs into the d_rpos / d_rsph the first one left. The decision margins of tests/reference_cases.py hold for both calls. A
grouped case is compared with the oracle's calls on has_plan masked to each range, as in tests/test_gpu_groups.py."""
import numpy as np
import pytest

import reference_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hdsm():
    from multi_agent_pkgs_amd import lib
    return lib


def _oracle(oracle, c, caps):
    N = c.n_hor
    full, ref, pv = np.zeros((c.n_inst, N + 1, 6)), np.zeros((c.n_inst, N, 6)), np.zeros(c.n_inst)
    for idx, mask in c.masked_calls():
        full[idx], ref[idx], pv[idx] = oracle.reference(c.prm(), c.cfg(), c.agent_id[idx], c.path[idx], c.n_path[idx], c.plans, mask,
                                                        vel_cap=None if caps is None else caps[idx])
    return full, ref, pv


def _compare(got, want, what):
    rel = 0.0
    for g, w, out in zip(got, want, ("ref_full", "ref", "path_vel")):
        err, scale = np.abs(g - w).max(), max(1.0, np.abs(w).max())
        assert err < 1e-10 * scale, (what, out, err, int(np.argmax(np.abs(g - w).reshape(len(g), -1).max(1))))
        rel = max(rel, err / scale)
    return rel


def _run(hdsm, oracle, name):
    c = rc.case(name)
    sol = hdsm.Solver(c.prm(), c.n_inst, c.n_rob)
    if c.groups is not None:
        sol.set_groups(c.groups)
    rel = 0.0
    for caps in (c.caps, c.other_caps()):
        got = sol.reference(c.cfg(), c.agent_id, c.path, c.n_path, c.plans, c.has_plan, vel_cap=caps)
        want = _oracle(oracle, c, caps)
        rel = max(rel, _compare(got, want, (name, "capped" if caps is not None else "no cap")))
        if c.exact and caps is not None:
            assert got[2].tobytes() == want[2].tobytes() == caps.tobytes()
    sol.close()
    line = f"{name}: NT = {c.nt}, largest relative difference {rel:.2e}"
    if rc.family_of(name) == "capacity":
        st = rc.sphere_stats(c)
        line += (f", survivors min / median / max {st['survivors'].min()} / {np.median(st['survivors']):.0f} / {st['survivors'].max()}"
                 f" of {c.n_rob - 1}, largest first filling {st['first_filling'].max()}")
    print(line)


@pytest.mark.parametrize("name", rc.names("capacity"))
def test_capacity(hdsm, oracle, name):
    """The survivor list at and behind its 2048 entries: NT = 64 without a drain (2048 agents), one id behind it (2049), a sixth trip
    (2561); NT = 256 with one drain (2049) and two (4097); tight balls (nearly every neighbour survives), sparse swarms (the crafted
    instances: the only close neighbour is id 2047 / 2048 / n_rob - 1; the closest sphere is not the setter), and the tight ball
    under three groups, one of 2061 ids from id 70 on. Instances: a shuffled subset of the ids."""
    _run(hdsm, oracle, name)


@pytest.mark.parametrize("name", rc.names("polyline"))
def test_polyline(hdsm, oracle, name):
    """pmax = 80: n_path 1, 2, 63, 64 (the last in LDS), 65, 80 (global memory), points 0.1 m apart, paths that run out, duplicate
    points, path_vel_dec 0 / 0.5 / 100, caps 0 / 0.05 / 0.11 / 5 / 50 / none, both launch forms; the walk that lands exactly."""
    _run(hdsm, oracle, name)


@pytest.mark.parametrize("name", rc.names("config"))
def test_configurations(hdsm, oracle, name):
    """sens_dist < 0 and path_vel_max < path_vel_min (every pair evaluated), weights that fall with the step, coincident agents, two
    neighbours equally far, instances whose agent has no plan, agents behind the partition; 300 and 20 instances of 300 agents."""
    _run(hdsm, oracle, name)


@pytest.mark.parametrize("name", rc.names("nonfinite"))
def test_non_finite_plans(hdsm, oracle, name):
    """has_plan = 1 and a plan with NaN or +-inf in it: a NaN step limits nothing, an infinite one gives v_max, the neighbour's
    finite steps count (a-e), and so do the neighbours met after it (f)."""
    _run(hdsm, oracle, name)


def test_device_entry_clamps_n_path(hdsm, oracle):
    """hdsm_reference_device takes n_path of 0, -3 and pmax + 5 (the host entry rejects them) as 1, 1 and pmax: compared with the
    oracle on the clamped counts. Twice on one handle, without and with vel_cap."""
    import torch
    c = rc.case("clamp")
    N, dev = c.n_hor, torch.device("cuda", 0)

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    sol = hdsm.Solver(c.prm(), c.n_inst, c.n_rob)
    d_id, d_path, d_np, d_plans, d_has = up(c.agent_id), up(c.path), up(c.n_path_device), up(c.plans), up(c.has_plan)
    caps = np.random.default_rng(9).uniform(6.0, 12.0, c.n_inst)
    rel = 0.0
    for cap in (None, caps):
        full, ref, pv = (torch.full(s, np.nan, dtype=torch.float64, device=dev) for s in ((c.n_inst, N + 1, 6), (c.n_inst, N, 6), (c.n_inst,)))
        sol.reference_device(c.cfg(), d_id, d_path, d_np, d_plans, d_has, full, ref, pv, vel_cap=None if cap is None else up(cap))
        torch.cuda.synchronize()
        rel = max(rel, _compare([t.cpu().numpy() for t in (full, ref, pv)], _oracle(oracle, c, cap), ("clamp", cap is not None)))
    sol.close()
    print(f"clamp: NT = {c.nt}, largest relative difference {rel:.2e}")
