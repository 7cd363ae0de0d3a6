#!/bin/bash
# A/B builds: variants/liblorb_<name>.so with the BA units (lorb_ba*.hip) compiled with extra flags,
# the rest from the regular build.  Variants live outside the package directory (lorb_slam_amd/ holds
# one library).
# usage: tools/build_variant.sh NAME "-DFLAG=1 ..."
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R/lorb_slam_amd/csrc" || exit 1
make -s || exit 1
mkdir -p _build_v "$R/variants"
objs=()
pids=()
for src in lorb_ba*.hip; do
  o=_build_v/${src%.hip}_$1.o
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off $2 -c "$src" -o "$o" &
  pids+=($!)
  objs+=("$o")
done
for p in "${pids[@]}"; do wait "$p" || exit 1; done
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared -o "$R/variants/liblorb_$1.so" "${objs[@]}" \
  $(ls _build/*.o | grep -v '/lorb_ba') -lamdhip64 -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
