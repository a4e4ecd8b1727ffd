#!/bin/bash
# needs the diagnostic build: make -C climate_toolbox_amd/csrc diag  (the production library has no knobs)
# usage: tools/split_ablate.sh [LIB] [bench args...]   (LIB: a library under climate_toolbox_amd/lib, default libwagg_diag.so)
# diagnostic: times dense_split_kernel<23> (c2-dense) under the WAGG_SPLIT_DBG knobs (bit0 = no W loads and no X LDS-DMA
# in the k-loop, bit2 = no per-tile wait or barrier, bit3 = no split arithmetic: DBGS="0 8 1 9" for the split's share);
# results are wrong with a knob set, only the time matters.  A plan that holds the f16 image of W runs the image variants of
# DBG 0 / 1 / 4 / 5 (bit3 is the split's own knob and reads the fp32 W); WAGG_SPLIT_IMG=0 in front takes the in-register
# split instead, in the same process and on the same plan
LIB=${1:-libwagg_diag.so}; shift
for d in ${DBGS:-0 1 4 5}; do
  echo -n "DBG=$d "; WAGG_SPLIT_DBG=$d timeout -k 10 300 python3 bench.py --full --diag-lib $LIB --steps 10 --warmup 3 --no-secondary --no-cpu-baseline "$@" 2>/dev/null | python3 -c "import json,sys; r=json.loads(sys.stdin.readline()); print('kernel_ms_median', round(r['roofline']['kernel_ms_median'],3), 'frac', round(r['roofline']['frac'],4), 'step_ms', round(r['ms_per_step'],3))" || exit 1
done
