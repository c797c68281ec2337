#!/bin/bash
# tools/dev/clusterprof.sh [out.txt] — the split of E21's nine launches: rocprofv3 kernel trace of ONE list of
# tools/dev/clusterbench.py per run (a run of its own, no counters), the k_cl_* rows of the kernel statistics per list.
# Every run under its own timeout; nothing is started after a run that fails.
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${1:-/dev/stdout}
for name in converged two_modes spread; do
  D=$(mktemp -d)
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $D -o s -- python $R/tools/dev/clusterbench.py --list $name 5 > $D/log.txt 2>&1 || { echo "$name: exit status $? (log: $D/log.txt)"; tail -5 $D/log.txt; exit 1; }
  F=$(find $D -name '*kernel_stats.csv' | head -1)
  { echo "== $name: kernel statistics of 6 calls (1 warm-up + 5 timed), columns as rocprofv3 writes them"; head -1 "$F"; grep -E 'k_cl_|k_bins_' "$F"; } >> $OUT
done
