"""CPU tests of the Python binding itself (multi_agent_pkgs_amd/lib.py): the signatures it reads from the three headers, the typed
array pointers, NULL, and the text an HdsmError carries per family of functions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from multi_agent_pkgs_amd import lib, swarm
from multi_agent_pkgs_amd.params import HdsmParams, agile_params, default_map_config
from abi_headers import ROOT, declared_functions  # a regular expression of its own, independent of the binding's parser

HEADERS = ("hdsm.h", "hdsm_swarm.h", "hdsm_stats.h")


def _argument_counts():
    """Commas + 1 inside the parentheses of each declaration, straight from the header text."""
    counts = {}
    for h in HEADERS:
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        for name, args in re.findall(r"\b(hdsm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
            counts[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return counts


def test_every_declared_function_gets_its_signature_from_the_headers():
    L = lib.load()
    names = sorted(n for h in HEADERS for n in declared_functions(h))
    assert len(names) == len(set(names)) >= 105
    assert sorted(lib.EXPORTS) == names
    counts = _argument_counts()
    assert sorted(counts) == names
    for n in names:
        fn = getattr(L, n)
        assert fn.argtypes is not None and len(fn.argtypes) == counts[n], n
    assert L.hdsm_stats_create.restype is C.c_void_p
    assert L.hdsm_map_region_scratch_bytes.restype is C.c_size_t and L.hdsm_poly_octa3d_scratch_bytes.restype is C.c_size_t
    for n in ("hdsm_last_error", "hdsm_map_last_error", "hdsm_corridor_last_error", "hdsm_dswarm_last_error"):
        assert getattr(L, n).restype is C.c_char_p, n
    assert L.hdsm_destroy.restype is None
    assert L.hdsm_create.argtypes[0] is C.POINTER(HdsmParams) and L.hdsm_swarm_create.argtypes[1] is C.POINTER(swarm.SwarmConfig)
    assert L.hdsm_swarm_flight_report.argtypes[1].dtype == lib.FLIGHT_REPORT and L.hdsm_dswarm_last_audit_round.argtypes[1].dtype == lib.AUDIT_ROUND
    assert L.hdsm_poly_octa3d_scratch_bytes(3) > 2 ** 16          # a size_t, not what is left of it in an int


def test_the_parser_reads_arrays_as_pointers_and_refuses_a_type_it_does_not_know():
    sig = lib.parse_declarations("/* int hdsm_no(int x); */\n#define HDSM_Y(a) a\nvoid hdsm_a(void);\n"
                                 "const char* hdsm_b(const int32_t dim[3], double* x,\n  float ms[7]); // int hdsm_c(void);\n")
    assert list(sig) == ["hdsm_a", "hdsm_b"] and sig["hdsm_a"] == (None, [])
    ret, (dim, x, ms) = sig["hdsm_b"]
    assert ret is C.c_char_p and dim.dtype == np.int32 and x.dtype == np.float64 and ms.dtype == np.float32
    with pytest.raises(TypeError) as e:
        lib.parse_declarations("int hdsm_x(const long double* p);")
    assert "hdsm_x" in str(e.value) and "long double" in str(e.value)
    with pytest.raises(TypeError) as e:
        lib.parse_declarations("uint16_t hdsm_y(void);")
    assert "hdsm_y" in str(e.value) and "uint16_t" in str(e.value)


def test_an_array_of_another_dtype_or_layout_never_reaches_the_library():
    L, cfg = lib.load(), default_map_config()
    dim, lo, bd = (np.array(v, np.int32) for v in ((40, 37, 23), (3, 4, 5), (2, 2, 2)))
    out = [np.full(3, -7, np.int32) for _ in range(4)]
    with pytest.raises(C.ArgumentError):
        L.hdsm_map_region_extent(cfg, dim.astype(np.int64), lo, bd, *out)
    with pytest.raises(C.ArgumentError):
        L.hdsm_map_region_extent(cfg, dim, lo, np.array([2, 9, 2, 9, 2, 9], np.int32)[::2], *out)
    with pytest.raises(C.ArgumentError):
        L.hdsm_map_region_extent(agile_params(10), dim, lo, bd, *out)      # another struct than hdsm_map_config
    assert all((o == -7).all() for o in out)
    assert L.hdsm_map_region_extent(cfg, dim, lo, bd, *out) == 0 and (out[1] >= bd).all()
    assert [o.tolist() for o in out] == [o.tolist() for o in lib.map_region_extent(cfg, (40, 37, 23), [3, 4, 5], (2, 2, 2))]
    # a shard of two agents, the raw function: float32 goals, then a non-contiguous float64 view of the right shape
    starts, goals = np.zeros((2, 3)), np.array([[5.0, 0.0, 1.0], [0.0, 5.0, 1.0]])
    shard = swarm.SwarmShard(agile_params(10), swarm.default_swarm_config(), 2, 0, starts, goals)
    with pytest.raises(C.ArgumentError):
        L.hdsm_swarm_set_goals(shard.h, goals.astype(np.float32))
    with pytest.raises(C.ArgumentError):
        L.hdsm_swarm_set_goals(shard.h, np.zeros((2, 6))[:, ::2])
    assert L.hdsm_swarm_set_goals(shard.h, goals) == 0
    shard.set_goals(goals.astype(np.float32))                              # the wrapper converts, as it always did


def test_none_is_null_and_ctypes_objects_pass_as_before():
    L = lib.load()
    assert L.hdsm_swarm_update_world(None, None, None, None) == lib.HDSM_ERR_BAD_ARG
    assert L.hdsm_map_region_extent(None, None, None, None, None, None, None, None) == lib.HDSM_ERR_BAD_ARG
    p = HdsmParams()
    L.hdsm_default_params(C.byref(p), 10)
    assert p.n_hor == 10
    arr, dim = (C.c_int32 * 3)(1, 1, 1), np.array((8, 8, 8), np.int32)
    wlo = np.zeros(3, np.int32)
    assert L.hdsm_map_region_extent(default_map_config(), dim.ctypes.data_as(C.POINTER(C.c_int32)), arr, arr, wlo, None, None, None) == 0
    assert (wlo == 0).all()


def test_an_error_carries_the_text_of_its_family():
    """The strings are those of a run of the same calls before the binding was rewritten."""
    with pytest.raises(lib.HdsmError) as e:                                # solver family: hdsm_last_error
        lib.Solver(agile_params(10), 0, 4)
    assert e.value.code == lib.HDSM_ERR_BAD_ARG and str(e.value) == "hdsm error -1: max_instances/n_rob_max must be >= 1"
    with pytest.raises(lib.HdsmError) as e:                                # map family: hdsm_map_last_error
        lib.map_region_extent(default_map_config(potential_dist=3.5), (40, 37, 23), [0, 0, 0], [1, 1, 1])
    assert e.value.code == lib.HDSM_ERR_BAD_ARG and str(e.value) == "hdsm error -1: mask radius above 9 voxels"
    with pytest.raises(lib.HdsmError) as e:
        lib.map_region_extent(default_map_config(), (40, 37, 23), [39, 0, 0], [2, 1, 1])
    assert str(e.value) == "hdsm error -1: the edit box does not lie inside the grid"
    shard = swarm.SwarmShard(agile_params(10), swarm.default_swarm_config(), 2, 0, np.zeros((2, 3)), np.ones((2, 3)))
    with pytest.raises(lib.HdsmError) as e:                                # the swarm functions report their own name
        shard.set_path_clearance(100.0)
    assert e.value.code == lib.HDSM_ERR_BAD_ARG and str(e.value) == "hdsm error -1: hdsm_swarm_set_path_clearance"
    with pytest.raises(lib.HdsmError) as e:
        shard.flight_report()
    assert str(e.value) == "hdsm error -1: hdsm_swarm_flight_report"
    with pytest.raises(lib.HdsmError) as e:
        swarm.poly_octa3d(np.zeros((20, 67, 67), np.int8), (33, 33, 10), max_rows=4)
    assert e.value.code == lib.HDSM_ERR_CAPACITY and str(e.value) == "hdsm error -4: hdsm_poly_octa3d"
    with pytest.raises(lib.HdsmError) as e:
        lib.local_path_host(None, (10, 10, 10), np.zeros((1, 3)), [0], np.zeros((1, 3)), np.zeros((1, 3)), np.ones((1, 3)), pmax=1)
    assert str(e.value) == "hdsm error -1: hdsm_local_path_host"
