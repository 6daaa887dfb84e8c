"""The built gfx950 code objects of libhdsm.so, read on the CPU: no solver kernel may use scratch memory.

Round 3 removed every scratch access from the solver kernels (hoisted addresses spilled across the active-set run), round 5 brought
20 B/lane back unnoticed (a loop-invariant 16-byte zero hoisted in front of the tree loop and spilled: +1.9 MB of HBM writes per
launch). The kernel descriptors in the library say what the hardware will be asked for (`.private_segment_fixed_size`), so the
regression is caught here, without a GPU and without recompiling."""
import os
import shutil

import pytest

from kernel_elf import LIB, _kernel_descriptors

def test_no_solver_kernel_uses_scratch(tmp_path):
    if not os.path.exists(LIB):
        pytest.skip("libhdsm.so not built")
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no ROCm toolchain")
    desc = _kernel_descriptors(tmp_path)
    solver = {k: v for k, v in desc.items() if "k_replan" in k}
    # every launch shape DESIGN.md lists must be in the library
    for shape in ("8k_replanILi32ELi1536ELi256", "8k_replanILi48ELi1024ELi256", "12k_replan_duoILi32ELi768ELi256", "12k_replan_triILi32ELi384ELi128",
                  "13k_replan_quadILi32ELi256ELi128", "14k_replan_duo48ILi48E"):
        assert any(shape in k for k in solver), shape
    bad = {k: v["private_segment_fixed_size"] for k, v in solver.items() if v.get("private_segment_fixed_size", 0) != 0}
    assert not bad, "solver kernels with scratch (bytes per lane): %r" % bad
    # the kernels that share a CU must fit the register budget of their residency: 2 waves per SIMD -> 256 registers
    for k, v in solver.items():
        if any(t in k for t in ("k_replan_quad", "k_replan_tri", "k_replan_duoILi32")):
            assert v["vgpr_count"] <= 256, (k, v)
    # the device-corridor and swarm kernels were scratch-free on their hot paths too; record what the others use
    others = {k: v.get("private_segment_fixed_size", 0) for k, v in desc.items() if "k_replan" not in k}
    assert len(others) >= 10
