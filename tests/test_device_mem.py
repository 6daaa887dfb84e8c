"""csrc/device_mem.h (the owners) and csrc/hdsm_handle.h (the solver handle built from them) on the CPU: tests/device_mem_check.cpp is a stand-alone program
that includes the header with its host seam (HDSM_DEVICE_MEM_HOST: malloc'ed blocks, a count of the live ones, a knob that fails
the k-th allocation) and asserts the ownership rules itself; it is built here with the address and undefined-behaviour sanitizers
and must exit 0. Nothing of it is loaded into Python and nothing of the HIP runtime is linked."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INC = "/opt/rocm/include"


def test_device_mem_ownership_on_the_host(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    if not os.path.exists(os.path.join(ROCM_INC, "hip", "hip_runtime_api.h")):
        pytest.skip("no ROCm headers")
    exe = str(tmp_path / "device_mem_check")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-DHDSM_DEVICE_MEM_HOST", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INC,
                            os.path.join(HERE, "device_mem_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    # (every leak check is the program's own count of live blocks; the sanitizer's leak pass needs ptrace, which containers often refuse)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks held" in run.stdout
