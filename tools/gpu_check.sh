# GPU suite, then the three variants' bench lines with their stage times:  bash tools/gpu_check.sh [OUT_DIR]
R=$(cd "$(dirname "$0")/.." && pwd); O=${1:-${TMPDIR:-/tmp}/gpu_check}; mkdir -p $O
cd $R && timeout 900 python -m pytest tests -m gpu -q -x > $O/pytest_gpu.log 2>&1; echo pytest_exit=$?; tail -3 $O/pytest_gpu.log
cd /tmp && export TMPDIR=/tmp
for v in surfel ewa plane; do timeout 300 python $R/bench.py --full --variant $v --steps 50 --warmup 5 --no-cpu-baseline > $O/bench_$v.json 2>/dev/null; python -c "import json;d=json.load(open('$O/bench_$v.json'));print('$v',d['value'],d['stage_ms'])"; done
