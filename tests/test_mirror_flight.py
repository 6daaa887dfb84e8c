"""The host mirror's side of the flight in and out of the device-resident loop (csrc/swarm_host.h, swarm_flight.cpp) on the CPU:
tests/mirror_flight_check.cpp is a stand-alone program that drives the C ABI of the mirror, hands a mirror the pieces of its own flight
through the adopt functions hdsm_dswarm_download uses and asserts itself that nothing changes and that the refusals hold; it is built
here from the mirror's sources with the address and undefined-behaviour sanitizers and must exit 0. Nothing of it is loaded into Python
and nothing of the HIP runtime is linked."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "multi_agent_pkgs_amd", "csrc")
SOURCES = ["swarm_host.cpp", "swarm_router.cpp", "swarm_world.cpp", "swarm_models.cpp", "swarm_flight.cpp",
           "stats_host.cpp", "audit_host.cpp", "path_host.cpp"]


def test_mirror_adopts_its_own_flight_unchanged(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "mirror_flight_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-pthread",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "mirror_flight_check.cpp")] + [os.path.join(CSRC, s) for s in SOURCES] + ["-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    # (the sanitizer's leak pass needs ptrace, which containers often refuse)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks held" in run.stdout
