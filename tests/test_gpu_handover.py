"""The flight across the hand-over between the host mirror and the device-resident loop on the MI355X (hdsm_dswarm_create takes the
mirror's flight over, hdsm_dswarm_download hands it back; csrc/dswarm_flight.cpp, csrc/swarm_flight.cpp). Two mirrors are built
identically — 6 agents, H = 10, one shard, in the open strip of the loop_cases world, groups of 2 and 4, path period 3, clearance on,
the audit on with two audited host rounds, commands on with a non-zero yaw0, one goal changed behind those rounds — and one of them goes
through a device loop and back with no round in between. Nothing of the flight may be lost or altered on the way: the two mirrors
answer every getter with the same bytes, and the host rounds flown after it are the same rounds (period 3 and the due agent make the
path step's phase show within three of them)."""
import ctypes as C

import numpy as np
import pytest

import corridor_oracle as co
import loop_cases as lc
from multi_agent_pkgs_amd import swarm
from multi_agent_pkgs_amd.lib import call
from flight_harness import device_loop, hdsm  # noqa: F401  (hdsm: the module's fixture)

pytestmark = pytest.mark.gpu

GROUPS = [0, 2, 6]
YAW0 = np.array([0.3, -0.2, 1.1, 2.5, -3.0, 0.7])


def _mirror(hdsm):  # noqa: F811
    prm, cfg = lc.shape_params(lc.SHAPES[0])
    s16, _ = lc.open_scene()
    starts = s16[[0, 1, 2, 8, 9, 10]]
    goals = starts[[4, 5, 3, 1, 2, 0]] + [0.0, 0.3, 0.0]
    sol, loop = device_loop(hdsm, prm, cfg, 6, starts=starts, goals=goals)
    grid, origin = lc.make_world()
    assert loop.set_world(grid, origin, route=False) == 0
    loop.pmax = 32
    sh = loop.shard
    sh.set_groups(GROUPS)
    sol.set_groups(GROUPS)          # the mirror's rounds call the solver themselves
    sh.set_path_period(3)
    sh.set_path_clearance(0.9)
    sh.set_audit(True, 1.25)
    sh.set_commands(True, yaw0=YAW0)
    for _ in range(2):
        loop.step()
    goals[3] += [0.0, 1.5, 0.0]
    sh.set_goals(goals)             # agent 3 is due in the next round; the path step's phase is 2 of 3
    return sol, loop


def _answers(shard):
    on, warn = C.c_int32(-1), C.c_double(-1.0)
    call("hdsm_swarm_get_audit", shard.h, C.byref(on), C.byref(warn))
    sp, pose, yaw = shard.commands()
    paths, n_path = shard.get_paths()
    return dict(agents=lc.agents_bytes(co.export_agents(shard)[0]), report=shard.flight_report().tobytes(), audit=(on.value, warn.value),
                setpoint=sp.tobytes(), pose=pose.tobytes(), yaw=yaw.tobytes(), paths=paths.tobytes() + n_path.tobytes())


def test_a_flight_through_the_device_loop_and_back_is_the_flight(hdsm):  # noqa: F811
    (sol_a, a), (sol_b, b) = _mirror(hdsm), _mirror(hdsm)
    before = _answers(a.shard)
    assert _answers(b.shard) == before                        # (the twins are twins)
    assert before["audit"] == (1, 1.25) and a.shard.flight_report()["rounds"].tolist() == [2] * 6
    assert np.frombuffer(before["yaw"]).all()                  # (a yaw the device loop must keep)

    dsw = swarm.DeviceSwarm(b.shard, sol_b)                    # take_over ...
    dsw.download(states=True)                                  # ... and hand_back, no round in between
    dsw.close()
    got = _answers(b.shard)
    for key, want in before.items():
        assert got[key] == want, key

    for r in range(3):
        out_a, out_b = a.step(), b.step()
        assert (out_a["status"] == out_b["status"]).all(), r
        got_a, got_b = _answers(a.shard), _answers(b.shard)
        for key, want in got_a.items():
            assert got_b[key] == want, (r, key)
    assert got_a["agents"] != before["agents"] and a.shard.flight_report()["rounds"].tolist() == [5] * 6
    sol_a.close(), sol_b.close()
