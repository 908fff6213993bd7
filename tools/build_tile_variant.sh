#!/bin/bash
# Builds lib/libcascadeclassifier_amd_<ty>_<threads>.so: the library with another cascade-kernel tile shape
# (window rows per tile x threads per block). Select it with CCAMD_LIB=<path>. Tuning experiments only.
# The Makefile knows which translation units size tiles (TILE_OBJ) and which objects make the library; the variant's
# objects go to a build directory of their own.
set -e
ty=$1; th=$2
make -C "$(dirname "$0")/../cascadeclassifier_amd/csrc" BUILD=build/tile_${ty}_${th} OUT_NAME=libcascadeclassifier_amd_${ty}_${th}.so \
  TILE_FLAGS="-DCC_TILE_Y=$ty -DCC_EVAL_THREADS=$th"
echo built cascadeclassifier_amd/lib/libcascadeclassifier_amd_${ty}_${th}.so
