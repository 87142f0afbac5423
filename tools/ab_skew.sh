# object-centric density (a few hundred tiles with very long lists): per-tile against global depth order.  bash tools/ab_skew.sh
R=$(cd "$(dirname "$0")/.." && pwd); cd /tmp
B="python $R/bench.py --full --no-cpu-baseline --no-method-iteration --no-graph-replay --steps 30 --warmup 6 --skew-frac 0.5"
for sc in 0.3 0.15 0.08; do for m in tile global; do
GSR_DEPTH_ORDER=$m $B --skew-scale $sc 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.read()); s=d['stage_ms']
print('scale $sc', '$m', d['value'], 'order', s['depth_order'], 'binning', s['binning'], 'fwd', s['blend_fwd'], 'bwd', s['blend_bwd'], 'mean', d['config']['gaussians_per_tile_mean'], 'max', d['config']['gaussians_per_tile_max'])"
done; done
