#!/bin/bash
# Tile-shape sweep of the specialised cascade kernel (variants built by tools/build_tile_variant.sh, each at the register
# budget it was built with: CC_EVAL_MIN_WAVES_PER_EU). Device pipeline only, 32 frames per launch; checks the rectangles of a
# small detection against the default build first (a variant that changes results is a bug, not a candidate).
run() {
  lib=$1
  [ -f "$lib" ] || return
  CCAMD_LIB=$lib CCAMD_CACHE_DIR= CCAMD_TRACE_HOST=1 python bench.py --steps 3 --warmup 1 --cpu-frames 0 --frames 32 --device-only --specialize 7 2> >(grep "resident blocks" >&2) | python -c "
import json,sys
d=json.loads(sys.stdin.readline()); print('$lib', 'eval_ms/32f', d['kernel_ms_per_step']['eval_ms'])"
}
L=cascadeclassifier_amd/lib
for v in "" _12_384 _8_512 _16_512 _16_256 _4_256 _6_384; do run $L/libcascadeclassifier_amd$v.so; done
