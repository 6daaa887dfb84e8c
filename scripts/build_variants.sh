#!/bin/bash
# builds libhdsm_<name>.so for each "name=DEFS" argument through csrc/Makefile (scripts/gpu_ab_builds.sh benches them)
csrc="$(dirname "$0")/../multi_agent_pkgs_amd/csrc"
for v in "$@"; do
  name=${v%%=*}; defs=${v#*=}
  ( make -C "$csrc" -s -B OUT=../libhdsm_$name.so DEFS="$defs" 2>&1 | grep -E "error" ; echo "built $name ($defs)" ) &
done
wait
