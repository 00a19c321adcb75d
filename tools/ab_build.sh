#!/bin/bash
# Baseline library for A/B timing: the source files in $SRC (default raster; SRC="ssim metrics" for several) with
# the headers beside them, all taken from git revision $REV (default HEAD), linked with the other current product
# objects -> lib/diag/libdgs_base.so
set -eu
cd "$(dirname "$0")/.."
SRC=${SRC:-raster}; REV=${REV:-HEAD}
PKG=deformable-3d-gaussians_amd
rm -rf $PKG/build_obj/abbase
mkdir -p $PKG/build_obj/abbase
git archive $REV $PKG/csrc include | tar -x -C $PKG/build_obj/abbase
SRC=$SRC SRCDIR=build_obj/abbase/$PKG/csrc bash tools/build_diag.sh base=
rm -rf $PKG/build_obj/abbase
