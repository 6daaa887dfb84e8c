"""Local ranks (ABI 1.9) on the CPU: the three new entry points as the binding reads them from the headers, the version, and the
bookkeeping of a local communicator group (csrc/local_group.h) under the address and undefined-behaviour sanitizers —
tests/local_group_check.cpp is a stand-alone program behind the host seam of csrc/device_mem.h (HDSM_DEVICE_MEM_HOST); nothing of it is
loaded into Python and nothing of the HIP runtime is linked. What the ranks fly is tested on the GPU (tests/test_gpu_local_ranks.py)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from multi_agent_pkgs_amd import lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INC = "/opt/rocm/include"


def test_the_new_entry_points_are_exported_with_their_argument_types():
    L = lib.load()
    ptrs = C.POINTER(C.c_void_p)
    want = {"hdsm_comm_create_local": [C.c_int32, ptrs, ptrs],                              # (world, handles, comms)
            "hdsm_dswarm_round_ranks": [C.c_int32, ptrs, ptrs, ptrs],                       # (world, dswarms, comms, hip_streams)
            "hdsm_dswarm_download_raw": [C.c_void_p, np.dtype(np.float64), np.dtype(np.float64)]}   # (dswarm, plans_all_raw, send_raw)
    for name, args in want.items():
        assert name in lib.EXPORTS, name
        restype, argtypes = lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == len(args), name
        for got, exp in zip(argtypes, args):
            assert (got.dtype == exp) if isinstance(exp, np.dtype) else (got is exp), (name, got, exp)
        assert list(getattr(L, name).argtypes) == list(argtypes) and hasattr(L, name)
    assert L.hdsm_version() >> 16 == 1 and L.hdsm_version() & 0xFFFF == 9


def test_an_array_of_pointers_the_callee_only_reads_is_a_pointer_to_pointers():
    sig = lib.parse_declarations("int hdsm_x(int32_t world, void* const* handles, void** comms, const double* p);")
    ret, (world, handles, comms, p) = sig["hdsm_x"]
    assert world is C.c_int32 and handles is C.POINTER(C.c_void_p) and comms is handles and p.dtype == np.float64
    with pytest.raises(TypeError):
        lib.parse_declarations("int hdsm_y(long* const* q);")


def test_null_arguments_are_refused_without_a_device():
    L = lib.load()
    assert L.hdsm_comm_create_local(0, None, None) == lib.HDSM_ERR_BAD_ARG
    one = (C.c_void_p * 1)()
    assert L.hdsm_comm_create_local(1, one, None) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_comm_create_local(1, one, one) == lib.HDSM_ERR_BAD_ARG and b"null handle of rank 0" in L.hdsm_last_error()
    assert L.hdsm_dswarm_round_ranks(1, None, None, None) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_dswarm_round_ranks(1, one, one, None) == lib.HDSM_ERR_BAD_ARG and b"rank 0" in L.hdsm_dswarm_last_error()
    assert L.hdsm_dswarm_download_raw(None, None, None) == lib.HDSM_ERR_BAD_ARG


def test_local_group_bookkeeping_under_the_sanitizers(tmp_path):
    """Groups of 1, 3 and 4 ranks, on one device and on several: created, left in every order, the last member frees the group; every
    allocation failing in turn leaves nothing behind. The program asserts it all itself and must exit 0."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    if not os.path.exists(os.path.join(ROCM_INC, "hip", "hip_runtime_api.h")):
        pytest.skip("no ROCm headers")
    exe = str(tmp_path / "local_group_check")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-DHDSM_DEVICE_MEM_HOST", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INC,
                            os.path.join(HERE, "local_group_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    # (every leak check is the program's own count of live blocks; the sanitizer's leak pass needs ptrace, which containers often refuse)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks held" in run.stdout
