#!/bin/bash
# Same-box A/B of two library builds over the scan workload of bench.py, outputs included: semcode_amd/_lib/libsemcode_hip.so (new)
# against semcode_amd/_lib/libsemcode_hip_base.so (a build of the parent commit), alternating new / parent / new / parent.
# scripts/ab_scan_report.py compares every dumped array bit for bit and the QPS of the headline and of each sweep point, with the
# difference between the two parent runs as the noise of the box.  Output: OUT/report.log
#   bash scripts/ab_scan_bench.sh [OUT]        (default build/ab_scan, which git ignores)
set -o pipefail
OUT=${1:-build/ab_scan}
L=semcode_amd/_lib
mkdir -p $OUT
cp $L/libsemcode_hip.so $L/new.so
i=0
for v in new base new base; do
    i=$((i + 1))
    if [ $v = new ]; then cp $L/new.so $L/libsemcode_hip.so; else cp $L/libsemcode_hip_base.so $L/libsemcode_hip.so; fi
    timeout -k 10 280 python bench.py --workload scan --full --no-cpu-baseline --dump-outputs $OUT/out_${i}_$v > $OUT/run_${i}_$v.log 2>&1
    rc=$?
    echo "== run $i $v rc=$rc"
    if [ $rc != 0 ]; then tail -20 $OUT/run_${i}_$v.log; cp $L/new.so $L/libsemcode_hip.so; exit $rc; fi
done
cp $L/new.so $L/libsemcode_hip.so
python scripts/ab_scan_report.py $OUT | tee $OUT/report.log
