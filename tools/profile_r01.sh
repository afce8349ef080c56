#!/bin/bash
# Regenerates the judged artifacts of the default bench (C2 single-pass): kernel stats, bench line, PMC traffic.
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/prof; mkdir -p $O
cd /tmp && export TMPDIR=/tmp
python $R/bench.py --full --steps 50 --warmup 10 > $O/bench_line.json 2> $O/bench.err
rm -rf /tmp/kt; rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/kt -- python $R/bench.py --full --steps 50 --warmup 10 --no-cpu-baseline --hot-only > $O/kt.log 2>&1
cp $(find /tmp/kt -name "*kernel_stats.csv" | head -1) $O/kernel_stats.csv
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf /tmp/pmc_$c; rocprofv3 --pmc $c --kernel-trace --output-format csv -d /tmp/pmc_$c -- python $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --hot-only > $O/pmc_$c.log 2>&1
  cp $(find /tmp/pmc_$c -name "*counter_collection.csv" | head -1) /tmp/cc_$c.csv
done
python - <<'PY' > $O/pmc_traffic.json
import csv, json, re, collections
per = collections.defaultdict(dict)
for c in ("FETCH_SIZE", "WRITE_SIZE"):
    acc = collections.defaultdict(float); n = collections.defaultdict(int)
    for r in csv.DictReader(open(f"/tmp/cc_{c}.csv")):
        if r["Counter_Name"] != c: continue
        m = re.search(r"(\w+_kernel)", r["Kernel_Name"])
        if not m: continue
        acc[m.group(1)] += float(r["Counter_Value"]); n[m.group(1)] += 1
    for k in acc:
        per[k][c + "_KB"] = acc[k] / n[k]; per[k]["launches_" + c] = n[k]
for k, v in per.items():
    v["hbm_bytes_corrected"] = (2 * v.get("FETCH_SIZE_KB", 0.0) + v.get("WRITE_SIZE_KB", 0.0)) * 1024
print(json.dumps({
    "command": "rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE --kernel-trace --output-format csv -- python bench.py --steps 10 --warmup 3 --no-cpu-baseline --hot-only  (two separate passes)",
    "workload": "C2 single-pass fused path (default bench): 128 views/launch, P=128, 256x256",
    "calibration": "same counters on a 256 MiB torch copy: FETCH_SIZE reads exactly 1/2 of the bytes (x2 applied), WRITE_SIZE exact (profiles/r01/pmc_traffic_C2_two_pass_v1.json)",
    "formula": "hbm_bytes_corrected = (2*FETCH_SIZE_KB + WRITE_SIZE_KB) * 1024",
    "per_launch": per}, indent=1))
PY
tail -1 $O/bench_line.json | head -c 600
