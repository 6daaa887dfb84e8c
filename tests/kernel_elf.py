"""The built gfx950 code objects of libhdsm.so, read on the CPU: kernel descriptors and segment sizes for the resource tests."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "multi_agent_pkgs_amd", "libhdsm.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _kernel_descriptors(tmp_path):
    """{kernel name: {field: int}} of every gfx950 code object bundled into the library."""
    objcopy, bundler, readelf = (os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))
    for t in (objcopy, bundler, readelf):
        if not os.path.exists(t):
            pytest.skip("ROCm LLVM tools not installed: " + t)
    fat = str(tmp_path / "fat.bin")
    subprocess.check_call([objcopy, "--dump-section", ".hip_fatbin=" + fat, LIB, str(tmp_path / "unused.so")])
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    assert starts, "no offload bundle in .hip_fatbin"
    out = {}
    for k, st in enumerate(starts):
        part = str(tmp_path / ("bundle%d.bin" % k))
        open(part, "wb").write(blob[st:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        co = str(tmp_path / ("dev%d.co" % k))
        subprocess.check_call([bundler, "--unbundle", "--type=o", "--input=" + part,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([readelf, "--notes", co], text=True)
        cur = None
        for ln in notes.splitlines():
            m = re.match(r"\s*\.(\w+):\s+(\S+)\s*$", ln)
            if not m:
                continue
            if m.group(1) == "name" and m.group(2).startswith("_Z"):
                cur = out.setdefault(m.group(2), {})
            elif cur is not None and m.group(1) in ("private_segment_fixed_size", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count",
                                                    "group_segment_fixed_size"):
                cur[m.group(1)] = int(m.group(2))
    return out


def _group_segments(tmp_path):
    """{kernel name: group_segment_fixed_size} read from the code objects _kernel_descriptors unbundled into tmp_path. In a kernel's
    note the group segment stands a few lines IN FRONT of its name (the keys are in alphabetical order), so the figure is searched
    backwards from the name, up to the end of the kernel before it."""
    out = {}
    for co in sorted(glob.glob(str(tmp_path / "dev*.co"))):
        lines = subprocess.check_output([LLVM + "/llvm-readelf", "--notes", co], text=True).splitlines()
        for i, ln in enumerate(lines):
            m = re.match(r"\s*\.name:\s+(_Z\S+)\s*$", ln)
            if not m:
                continue
            for back in lines[i - 1::-1]:
                g = re.match(r"\s*\.group_segment_fixed_size:\s+(\d+)\s*$", back)
                if g:
                    out[m.group(1)] = int(g.group(1))
                    break
                assert not re.match(r"\s*(- )?\.(symbol|vgpr_count|private_segment_fixed_size):", back), (m.group(1), back)
    return out


def _kernel_blocks(tmp_path):
    """{kernel name: {field: int}} read from the gfx950 code objects of the library with every field of a kernel's metadata entry
    (_kernel_descriptors reads the fields that follow `.name`; the group segment precedes it)."""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools):
        pytest.skip("libhdsm.so or the ROCm LLVM tools missing")
    fat = str(tmp_path / "fat.bin")
    subprocess.check_call([tools[0], "--dump-section", ".hip_fatbin=" + fat, LIB, str(tmp_path / "unused.so")])
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    out = {}
    for k, st in enumerate(starts):
        part, co = str(tmp_path / ("b%d.bin" % k)), str(tmp_path / ("d%d.co" % k))
        open(part, "wb").write(blob[st:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        subprocess.check_call([tools[1], "--unbundle", "--type=o", "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([tools[2], "--notes", co], text=True)
        for block in re.split(r"\n  - \.", notes)[1:]:
            name = re.search(r"^\s*\.name:\s+(\S+)\s*$", block, re.M)
            if name:
                out[name.group(1)] = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s{4}\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def assert_no_scratch_no_lds(tmp_path, substring, count=1, scalar_spills=False):
    """The `count` kernels of the built library whose name holds `substring`: no private segment, no spill, no group segment.
    scalar_spills: scalar registers parked in the lanes of a vector register are not held against the kernel."""
    assert os.path.exists(LIB), "libhdsm.so is not built"
    desc = _kernel_descriptors(tmp_path)
    mine = {k: v for k, v in desc.items() if substring in k}
    assert len(mine) == count, sorted(mine)
    lds = _group_segments(tmp_path)
    for k, v in mine.items():
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (k, v)
        assert scalar_spills or v.get("sgpr_spill_count", 0) == 0, (k, v)
        assert lds[k] == 0, (k, lds[k])
    print({k: dict(v, group_segment_fixed_size=lds[k]) for k, v in mine.items()})
