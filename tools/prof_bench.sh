#!/bin/bash
# usage (on the GPU box): tools/prof_bench.sh <tag>  -> prof_out/prof_<tag>/ + compact kernel table
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/prof_out
tag=${1:-x}
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $R/prof_out/prof_$tag -- python $R/bench.py --full --steps 10 --warmup 2 --no-overlap-figure > $R/prof_out/prof_$tag.json 2>/dev/null
cd $R
python - <<PY
import csv,glob,json
f=glob.glob('prof_out/prof_$tag/*/*kernel_stats.csv')[0]
for i,r in enumerate(csv.DictReader(open(f))):
    if i<22: print(r['Name'][:40].ljust(40), r['Calls'].rjust(5), r['TotalDurationNs'].rjust(10), r['AverageNs'][:9].rjust(10), r['MinNs'].rjust(7), r['MaxNs'].rjust(8))
d=json.load(open('prof_out/prof_$tag.json'))
print(d['ms_per_step'], d['kernel_ms_per_step'], d['parity_vs_oracle'])
PY
