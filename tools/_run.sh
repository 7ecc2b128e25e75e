OUT=${OUT:-build/bench_lines}; mkdir -p $OUT
rm -f $OUT/r02_bench_configs.jsonl $OUT/r02_bench_forcedist.jsonl
for w in headline cfg2 cfg2_panda cfg3 cfg3_poly cfg4 cfg5; do python bench.py --full --workload $w >> $OUT/r02_bench_configs.jsonl 2>>$OUT/r02_bench.err; done
MASTER_PORT=29561 python bench.py --full --force-dist --scaling strong --workload cfg3 >> $OUT/r02_bench_forcedist.jsonl 2>>$OUT/r02_bench.err
MASTER_PORT=29562 python bench.py --full --force-dist >> $OUT/r02_bench_forcedist.jsonl 2>>$OUT/r02_bench.err
MASTER_PORT=29563 python bench.py --full --force-dist --workload cfg5 --scaling strong >> $OUT/r02_bench_forcedist.jsonl 2>>$OUT/r02_bench.err
OUT=$OUT python - <<'PY'
import json, os
out = os.environ["OUT"]
for f in (out + "/r02_bench_configs.jsonl", out + "/r02_bench_forcedist.jsonl"):
    for l in open(f):
        d=json.loads(l)
        print(d["config"]["workload"][:10], d["scaling"], d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["kernel_ms"], (d.get("cpu_baseline") or {}).get("value"), d.get("multi"))
        for k,v in (d.get("variants") or {}).items(): print("    ",k,v["value"],v["ms_per_step"],v["gather_ms"])
PY
