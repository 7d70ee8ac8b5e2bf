#!/bin/bash
# The headline of two libraries, alternated in one job on one machine: usage  tools/ab_bench.sh <reps> <nameA=libA.so> <nameB=libB.so> [bench.py arguments]
# Prints every run's sweeps/s and, per library, median, min, max and spread ((max - min) / median).
R=$(cd "$(dirname "$0")/.." && pwd)
REPS=$1; A=$2; B=$3; shift 3
T=$(mktemp -d)
for rep in $(seq "$REPS"); do for kv in "$A" "$B"; do
  name=${kv%%=*}; lib=${kv#*=}
  export RC_LIB_PATH=$(cd "$(dirname "$lib")" && pwd)/$(basename "$lib")
  timeout -k 10 300 python3 "$R/bench.py" --gpus 1 --no-cpu-baseline --steps 200 "$@" 2> "$T/err.log" | tail -1 > "$T/line.json" || { echo "$name rep $rep failed"; tail -5 "$T/err.log"; exit 1; }
  python3 -c "import json, sys; print(json.load(open(sys.argv[1]))['value'])" "$T/line.json" >> "$T/$name.txt" || exit 1
done; done
for kv in "$A" "$B"; do
  name=${kv%%=*}
  python3 -c "
import statistics, sys
v = [float(x) for x in open(sys.argv[2])]
m = statistics.median(v)
print(sys.argv[1], ' '.join('%.0f' % x for x in v), 'median %.0f min %.0f max %.0f spread %.1f%%' % (m, min(v), max(v), 100 * (max(v) - min(v)) / m))" "$name" "$T/$name.txt"
done
rm -rf "$T"
