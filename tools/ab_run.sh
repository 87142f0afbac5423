#!/bin/bash
# A/B on one box: for each "name=libpath[:ENV=VAL]" argument prints it/s and blend stage times (ROUNDS alternating rounds, default 3).
# "name=@dir[:ENV=VAL]" runs the bench.py of the source tree in dir (relative to the repository) against that tree's own library: what a change that
# touches the Python side as well needs -- a parent LIBRARY under this tree's bridge is not the parent (and a library older than the null dL_dcov3D
# of the bridge must never be run under it).
# A bench run that fails or exceeds its time limit ends the script: nothing more is started on the device after it.
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd /tmp
for i in $(seq ${ROUNDS:-3}); do
  for spec in "$@"; do
    name=${spec%%=*}; rest=${spec#*=}; lib=${rest%%:*}; envs=""
    if [ "$rest" != "$lib" ]; then envs=$(echo ${rest#*:} | tr ':' ' '); fi
    if [ "${lib#@}" != "$lib" ]; then bench=$R/${lib#@}/bench.py; libenv="GSR_LIB_PATH="; else bench=$R/bench.py; libenv="GSR_LIB_PATH=$R/$lib"; fi
    env $envs $libenv timeout -k 10 ${BENCH_TIMEOUT:-240} python $bench --full --variant ${VARIANT:-surfel} --steps 60 --warmup 10 --no-cpu-baseline --no-method-iteration 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.read()); s=d['stage_ms']
print('$name', 'it/s', d['value'], 'fwd', round(s['blend_fwd'],4), 'bwd', round(s['blend_bwd'],4), 'pre', round(s['preprocess'],4), 'bin', round(s['binning'],4), 'pre_bwd', round(s['preprocess_bwd'],4))"
  done
done
