#!/bin/bash
# rows layout at world 1 through a 1-rank RCCL communicator: bench lines (own rows bypass the collectives / every row through the communicator),
# their kernel stats, and the full GPU suite a second time.  Usage: bash scripts/rows_final.sh [output directory]
D=${1:-rows_final_out}
mkdir -p $D
export DRX_BENCH_RCCL1=1
python bench.py --full --force-sharded --no-cpu-baseline --no-hr --no-configs > $D/rows_layout_world1_rccl.json 2> $D/rows1.err
python bench.py --full --force-sharded --no-self-bypass --no-cpu-baseline --no-hr --no-configs > $D/rows_layout_world1_rccl_all_remote.json 2> $D/rows2.err
unset DRX_BENCH_RCCL1
bash scripts/prof_rows.sh r04_rows_bypass > $D/prof_bypass.log 2>&1
bash scripts/prof_rows.sh r04_rows_allremote --no-self-bypass > $D/prof_allremote.log 2>&1
timeout -k 5 900 python -m pytest tests -q -m gpu -p no:cacheprovider > $D/gpu_tests_run2.log 2>&1; echo "suite rc=$?"; tail -1 $D/gpu_tests_run2.log
for f in $D/rows_layout_world1_rccl.json $D/rows_layout_world1_rccl_all_remote.json; do python -c "
import json,sys
d=json.loads([l for l in open('$f') if l.startswith('{')][-1]); print('$f', round(d['value']/1e6,1), round(d['ms_per_step'],4), d['phases_ms'])"; done
