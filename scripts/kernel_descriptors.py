#!/usr/bin/env python3
"""The kernel descriptors of one or two builds of libhdsm.so, read on the CPU (no GPU, no recompiling): registers, static LDS and
scratch of every gfx950 kernel, and what differs between two libraries.

    python scripts/kernel_descriptors.py multi_agent_pkgs_amd/libhdsm.so                      # one table
    python scripts/kernel_descriptors.py parent/libhdsm.so multi_agent_pkgs_amd/libhdsm.so    # the differences (+ --json out.json)

Fields: vgpr_count, sgpr_count, group_segment_fixed_size (static LDS; the solver kernels' instance state is DYNAMIC LDS and does
not show here), private_segment_fixed_size (scratch per lane), the two spill counts. Kernels are matched by their mangled names;
the hash suffix of anonymous-namespace symbols is stripped."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def descriptors(lib):
    objcopy, bundler, readelf = (os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([objcopy, "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "unused.so")])
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for k, st in enumerate(starts):
            part, co = os.path.join(tmp, "bundle%d.bin" % k), os.path.join(tmp, "dev%d.co" % k)
            open(part, "wb").write(blob[st:starts[k + 1] if k + 1 < len(starts) else len(blob)])
            subprocess.check_call([bundler, "--unbundle", "--type=o", "--input=" + part, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
            # a kernel's record is one item of the amdhsa.kernels list: its keys are sorted, so some fields stand BEFORE .name —
            # a record starts at its "- .key:" line and is filed under its name when the next one starts
            rec = {}

            def file_record():
                name = rec.get("name", "")
                if name.startswith("_Z") and "vgpr_count" in rec:
                    out[name] = {f: int(rec[f]) for f in FIELDS if f in rec}

            for ln in subprocess.check_output([readelf, "--notes", co], text=True).splitlines():
                m = re.match(r"(\s*)(-\s+)?\.(\w+):\s+(\S+)\s*$", ln)
                if not m:
                    continue
                if m.group(2) and len(m.group(1)) <= 2:  # (the list items of .args are indented deeper)
                    file_record()
                    rec = {}
                if m.group(3) == "name" and not m.group(4).startswith("_Z") and "name" in rec:
                    continue  # (an argument's .name)
                rec.setdefault(m.group(3), m.group(4))
            file_record()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("libs", nargs="+", help="one library (table) or two (old new: differences)")
    ap.add_argument("--json", help="write the result here")
    a = ap.parse_args()
    tabs = [descriptors(p) for p in a.libs[:2]]
    if len(tabs) == 1:
        res = tabs[0]
        for k in sorted(res):
            print(k, " ".join("%s=%d" % (f, res[k].get(f, 0)) for f in FIELDS))
    else:
        old, new = tabs
        res = {"kernels_old": len(old), "kernels_new": len(new), "only_old": sorted(set(old) - set(new)), "only_new": sorted(set(new) - set(old)),
               "same": sum(1 for k in old if k in new and old[k] == new[k]), "changed": {}}
        for k in sorted(set(old) & set(new)):
            if old[k] != new[k]:
                res["changed"][k] = {f: [old[k].get(f, 0), new[k].get(f, 0)] for f in FIELDS if old[k].get(f, 0) != new[k].get(f, 0)}
        print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
