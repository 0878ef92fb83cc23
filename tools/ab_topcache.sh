set -x
OUT=${OUT:-build/ab_topcache}; mkdir -p $OUT
for c in 1 0; do TWK_TOP_CACHE=$c timeout -k 10 200 python bench.py --full --no-cpu-baseline > $OUT/r02e_bench_cache$c.json 2>/dev/null; python - <<PY
import json
r=json.load(open("$OUT/r02e_bench_cache$c.json"))
rf=r["roofline"]
print("cache $c", r["value"], rf["kernel_ms_per_step"], rf["nodes_per_ray"], rf["lane_occupancy"]["node_step"], rf["frac"])
PY
done
