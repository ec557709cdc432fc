# Alternating bench runs of the C3 4-view step with 2 / 3 / 4 view streams (bench.py --streams).
# Results go to $OUT (default: bench_out/ under the repository root).
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p $OUT
for rep in 1 2; do for s in 2 3 4; do
  timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-train-step --no-graph --single-view-steps 0 --steps 100 --streams $s > $OUT/st_$s.$rep.json 2> $OUT/st_$s.$rep.err || exit 1
  python -c "
import json; d = json.load(open('$OUT/st_$s.$rep.json'))
print('streams $s value %8.1f sustained %8.1f' % (d['value'], d['sustained']['iters_s']))"
done; done
