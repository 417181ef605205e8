#!/bin/bash
# Same-box A/B of the batched IVF probes in two library builds: semcode_amd/_lib/libsemcode_hip.so (new) against
# semcode_amd/_lib/libsemcode_hip_base.so (a build of the parent commit).  Three timed runs per build, alternating (scripts/ab_ivf.py
# run), then the library's own phase times once per build (SC_IVF_TRACE), then the IVF_FLAT block of bench.py --full once per build.
# Every GPU step runs under its own time limit; the first failure ends the script.
#   bash scripts/ab_ivf.sh [OUT]        (default build/ab_ivf, which git ignores)  ->  OUT/report.log
set -o pipefail
OUT=${1:-build/ab_ivf}
L=semcode_amd/_lib
mkdir -p $OUT
rm -f $OUT/run_*.json
step() {  # step LIMIT LOG COMMAND...: the command under its time limit, its output in LOG; a failure ends the script
    local limit=$1 log=$2
    shift 2
    timeout -k 10 $limit "$@" > $log 2>&1
    local rc=$?
    echo "== $log rc=$rc"
    if [ $rc != 0 ]; then tail -20 $log; exit $rc; fi
}
i=0
for v in base new base new base new; do
    i=$((i + 1))
    lib=$L/libsemcode_hip.so
    [ $v = base ] && lib=$L/libsemcode_hip_base.so
    step 150 $OUT/run_${i}_$v.log python scripts/ab_ivf.py run $lib $OUT/run_${i}_$v.json
done
python scripts/ab_ivf.py report $OUT | tee $OUT/report.log
rc=$?
for v in base new; do
    lib=$L/libsemcode_hip.so
    [ $v = base ] && lib=$L/libsemcode_hip_base.so
    SC_IVF_TRACE=1 step 150 $OUT/trace_$v.log python scripts/ab_ivf.py trace $lib
    echo "# SC_IVF_TRACE, $v build" >> $OUT/report.log
    grep -E "^--- |\[ivf (list-major|coarse)\] Q" $OUT/trace_$v.log | sed -E 's/\| (D2H of probes|probe \+ D2H)/\n      | \1/' >> $OUT/report.log
done
for v in base new; do
    lib=$L/libsemcode_hip.so
    [ $v = base ] && lib=$L/libsemcode_hip_base.so
    step 420 $OUT/benchivf_$v.log python scripts/ab_ivf.py benchivf $lib
    echo "# IVF_FLAT block of bench.py --full, $v build" >> $OUT/report.log
    grep '^{' $OUT/benchivf_$v.log >> $OUT/report.log
done
exit $rc
