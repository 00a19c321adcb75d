#!/bin/bash
# Diagnostic variants of libdgs_hip.so (timing experiments, wrong results): the source files in $SRC (default
# mlp_split; a list in quotes for several) rebuilt with <flags> (e.g. -DFOO) and linked with the other product
# objects into lib/diag/libdgs_<name>.so; use with DGS_LIB=...   usage: [SRC="ssim metrics"] build_diag.sh name=flags ...
# (SRCDIR: another directory holding the sources and their headers, as tools/ab_build.sh extracts from a revision)
set -eu
cd "$(dirname "$0")/../deformable-3d-gaussians_amd"
SRC=${SRC:-mlp_split}
make -s -C csrc
mkdir -p lib/diag build_obj/diag
for v in "$@"; do
  name=${v%%=*}; flags=${v#*=}
  objs=$(ls build_obj/*.o); built=""
  for s in $SRC; do
    extra=""; [[ $s == mlp_split* ]] && extra="-mllvm -amdgpu-atomic-optimizer-strategy=None"  # as csrc/Makefile
    /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics $extra $flags -c ${SRCDIR:-csrc}/$s.hip -o build_obj/diag/${s}_$name.o
    objs=$(echo "$objs" | grep -v "/${EXCL:-$s}.o"); built="$built build_obj/diag/${s}_$name.o"
  done
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o lib/diag/libdgs_$name.so $objs $built
  echo "built lib/diag/libdgs_$name.so ($SRC $flags)"
done
