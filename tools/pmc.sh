#!/bin/bash
# HBM-side byte counters of the default bench, one rocprofv3 --pmc pass per
# counter (FETCH_SIZE uses 3 TCC slots and WRITE_SIZE 2, so they cannot share
# a pass), each pass under its own hard time limit.  Parsed by
# tools/pmc_parse.py into profiles/pmc_<workload>.json.
#   usage: bash tools/pmc.sh [workload]      (default sweep48)
set -o pipefail
OUT=${OUT:-bench_out}  # where the runs' files go (a path without spaces: it is used unquoted below)
case $OUT in *[[:space:]]*) echo "OUT must not contain spaces" >&2; exit 2 ;; esac
mkdir -p "$OUT"
WL=${1:-sweep48}
ROOT="${GRAFT_REPO_ROOT:-$(pwd)}"
cd /tmp && export TMPDIR=/tmp && cd "$ROOT" || exit 1
export TDA_BENCH_NO_SEQ=1  # traces hold only the pipelined batch (and its stage pass), not the one-call-at-a-time pass
for C in FETCH_SIZE WRITE_SIZE; do
    rm -rf $OUT/pmc_$C
    timeout -s KILL 120 rocprofv3 --pmc $C --output-format csv -d $OUT/pmc_$C -o run -- \
        python3 bench.py --full --workload $WL --steps 5 --warmup 1 --no-cpu --extra "" > $OUT/pmc_$C.txt 2>&1
    rc=$?
    echo "pmc $C rc=$rc"
    if [ $rc -ne 0 ]; then tail -20 $OUT/pmc_$C.txt; exit $rc; fi
done
python3 tools/pmc_parse.py --workload $WL --bench-out $OUT/pmc_FETCH_SIZE.txt $OUT/pmc_FETCH_SIZE $OUT/pmc_WRITE_SIZE > /dev/null
rc=$?
cp profiles/pmc_$WL.json $OUT/ 2>/dev/null  # a copy next to the passes it was parsed from
exit $rc
