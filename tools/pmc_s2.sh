#!/bin/bash
# Instruction and cycle counters of the headline row reduction, one counter-collection run per library (no tracing beside it).
# usage: tools/pmc_s2.sh <out dir> <name=lib.so> [<name=lib.so> ...]   ("name=" alone: the in-tree build)
# RC_PMC_COUNTERS="SQ_WAIT_ANY SQ_WAVE_CYCLES SQ_INSTS_VMEM_RD" collects other counters than the default four (one pass: at most what the SQ holds at once)
# Prints per kernel and counter the mean per launch; the raw csv files stay under <out dir>/<name>/.
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "$1" && cd "$1" && pwd); shift
export RC_BENCH_SETTLE_MS=${RC_BENCH_SETTLE_MS:-50}
for kv in "$@"; do
  name=${kv%%=*}; lib=${kv#*=}
  if [ -n "$lib" ]; then export RC_LIB_PATH=$(cd "$(dirname "$lib")" && pwd)/$(basename "$lib"); else unset RC_LIB_PATH; fi
  ( cd /tmp && TMPDIR=/tmp timeout -k 10 300 rocprofv3 --pmc ${RC_PMC_COUNTERS:-SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES} --output-format csv -d "$OUT/$name" -o r -- \
      python3 "$R/bench.py" --gpus 1 --no-cpu-baseline --steps 30 --warmup 5 > "$OUT/$name.log" 2>&1 ) || { echo "$name: counter run failed ($?)"; tail -5 "$OUT/$name.log"; exit 1; }
  python3 - "$OUT/$name" "$name" <<'PY'
import collections, csv, glob, sys
acc = collections.defaultdict(lambda: [0.0, 0])
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for row in csv.DictReader(open(f)):
        k = row["Kernel_Name"].split("(")[0][:40]
        if "k_bulk" in k or "k_resolve" in k:
            a = acc[(k, row["Counter_Name"])]; a[0] += float(row["Counter_Value"]); a[1] += 1
for (k, c), (v, cnt) in sorted(acc.items()):
    print(f"{sys.argv[2]:12s} {k:34s} {c:18s} per-launch {v / cnt:14.1f}  (launches {cnt})")
PY
done
