#!/bin/bash
# usage: tools/prof_variants.sh "0 1 2 3 4 7" <output dir>   — rocprofv3 kernel stats of bench.py --full under RC_DEBUG_FLAGS ablations
R=$GRAFT_REPO_ROOT
O=$(mkdir -p "${2:?usage: tools/prof_variants.sh <flags> <output dir>}" && cd "$2" && pwd)
cd /tmp && export TMPDIR=/tmp
for f in $1; do
  export RC_DEBUG_FLAGS=$f
  rocprofv3 --kernel-trace --stats --output-format csv -d $O/abl_$f -o b -- python3 $R/bench.py --full --steps 50 --warmup 5 --no-cpu-baseline > $O/abl_$f.json 2> $O/abl_$f.err
  echo "== flags=$f"; grep -E "k_resolve|k_bulk|k_zero" $O/abl_$f/b_kernel_stats.csv | cut -d, -f1-4,6,7
  python3 -c "import json;d=json.load(open('$O/abl_$f.json'));print('sweeps/s',round(d['value']),'ms/step',round(d['ms_per_step'],4),'bulk_ms',round(d['roofline']['avg_launch_ms'],4))"
done
