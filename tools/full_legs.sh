#!/bin/bash
# The other legs of bench.py --full for two libraries, alternated: usage  tools/full_legs.sh <reps> <out dir> <nameA=libA.so> <nameB=libB.so>
# (default-options chains and the 512-slot window switched off; the other configurations — config 5 — in the first repetition only)
R=$(cd "$(dirname "$0")/.." && pwd)
REPS=$1; OUT=$(mkdir -p "$2" && cd "$2" && pwd); shift 2
export RC_BENCH_NO_DEFAULTS=1 RC_BENCH_NO_KCAP512=1 RC_BENCH_WINDOWS=2
for rep in $(seq "$REPS"); do for kv in "$@"; do
  name=${kv%%=*}; lib=${kv#*=}
  export RC_LIB_PATH=$(cd "$(dirname "$lib")" && pwd)/$(basename "$lib")
  if [ "$rep" -gt 1 ]; then export RC_BENCH_NO_OTHER_CONFIGS=1; else unset RC_BENCH_NO_OTHER_CONFIGS; fi
  timeout -k 10 280 python3 "$R/bench.py" --gpus 1 --full --no-cpu-baseline --steps 200 2> "$OUT/full_${name}_$rep.err" | tail -1 > "$OUT/full_${name}_$rep.json" || { echo "$name rep $rep failed"; tail -5 "$OUT/full_${name}_$rep.err"; exit 1; }
  python3 - "$name" "$rep" "$OUT/full_${name}_$rep.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[3]))
def find(o, key):
    if isinstance(o, dict):
        if key in o:
            return o[key]
        for v in o.values():
            r = find(v, key)
            if r is not None:
                return r
    return None
m = find(d, "moving_regime") or {}
c5 = find(d, "config5_N32768_K200_32bit") or {}
f = lambda x: "n/a" if x is None else "%.0f" % x
print(sys.argv[1], sys.argv[2], "value", f(d.get("value")), "incremental_mode_sweeps_per_s_rank0", f(find(d, "incremental_mode_sweeps_per_s_rank0")),
      "moving sweeps_per_s", f(m.get("sweeps_per_s")), "incremental_mode", f(m.get("sweeps_per_s_incremental_mode")), "blocking", f(m.get("sweeps_per_s_blocking")),
      "changes/sweep %.1f" % m.get("label_changes_per_sweep", float("nan")), "config5 sweeps_per_s", c5.get("sweeps_per_s", c5.get("error", "n/a")))
PY
done; done
