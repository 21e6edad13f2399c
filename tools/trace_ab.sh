#!/bin/bash
# Kernel traces of bench.py's CG under several knob settings (one rocprofv3
# run each):  tools/trace_ab.sh "39=0" "40=4" ...   -> $MX_OUT/tab/<tag>/
# (default out/tab under the repository root)
set -eo pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${MX_OUT:-$R/out}/tab
export TMPDIR=/tmp
for k in "$@"; do
  tag=$(echo "k$k" | tr '=+' '__')
  mkdir -p $O/$tag
  (cd "$TMPDIR" && MXSOLVE_KNOBS=$k timeout -k 10 120 rocprofv3 --kernel-trace -f csv -d $O/$tag -o run -- python3 $R/bench.py --full --steps 200 --warmup 5 --no-cpu --no-solve > $O/$tag.log 2>&1)
  echo "== $k $(grep '^{' $O/$tag.log | tail -n 1 | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["value"], d["roofline"]["avg_launch_ms"])')"
  python3 $R/tools/trace_medians.py $O/$tag > $O/$tag.med
  sed -n 1,6p $O/$tag.med
done
