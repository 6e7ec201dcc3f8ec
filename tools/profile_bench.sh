#!/bin/bash
# rocprofv3 kernel trace + stats of the default bench -> $OUT/prof_trace
#   usage: bash tools/profile_bench.sh [workload] [extra bench args]
set -o pipefail
OUT=${OUT:-bench_out}  # where the runs' files go (a path without spaces: it is used unquoted below)
case $OUT in *[[:space:]]*) echo "OUT must not contain spaces" >&2; exit 2 ;; esac
mkdir -p "$OUT"
WL=${1:-sweep48}
shift
ROOT="${GRAFT_REPO_ROOT:-$(pwd)}"
cd /tmp && export TMPDIR=/tmp && cd "$ROOT" || exit 1
export TDA_BENCH_NO_SEQ=1  # traces hold only the pipelined batch (and its stage pass), not the one-call-at-a-time pass
rm -rf $OUT/prof_$WL
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$WL -o run -- \
    python3 bench.py --full --workload $WL --steps 20 --warmup 3 --no-cpu "$@" > $OUT/prof_$WL.txt 2>&1
rc=$?
echo "rocprof rc=$rc"
tail -1 $OUT/prof_$WL.txt
find $OUT/prof_$WL -name "*kernel_stats.csv" -exec cp {} $OUT/kernel_stats_$WL.csv \;
exit $rc
