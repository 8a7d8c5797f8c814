#!/bin/bash
# A/B/C... of compile-time variants on ONE GPU box (boxes of the pool differ by up to 30 %).
# usage: bash tools/ab_variants.sh "name:-DFLAG=1 -DOTHER=0" "name2:" ... -- [bench.py arguments]
# Builds one library per variant (tools/probes/lib_<name>.bin) in parallel, then tools/ab.py cycles through them twice on this box.
# AB_BUILD_ONLY=1: build and print the tools/ab.py call instead, to be run where the GPU is (the .bin files travel with the tree).
set -e
VARIANTS=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do VARIANTS+=("$1"); shift; done
[ "$1" == "--" ] && shift
LIBS=()
for v in "${VARIANTS[@]}"; do
  name="${v%%:*}"; flags="${v#*:}"
  LIBS+=(--lib "$name=tools/probes/lib_$name.bin")
  ( /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wno-unused-value $flags -o tools/probes/lib_$name.bin \
      bipedal_control_amd/csrc/{solver.hip,wbc.hip,capi.cpp,info_tree.cpp,urdf_tree.cpp,robot_model.cpp,reference_gen.cpp,device_model.cpp} > /tmp/ab_$name.log 2>&1 || echo "BUILD FAILED $name" ) &
done
wait
CYCLE=(python tools/ab.py "${LIBS[@]}" --args "$*" --limit 200 -- python bench.py --full --steps 30 --warmup 3 --cpu-sample 0)
if [ -n "$AB_BUILD_ONLY" ]; then printf '%q ' "${CYCLE[@]}"; echo; else "${CYCLE[@]}"; fi
