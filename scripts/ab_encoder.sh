#!/bin/bash
# Same-box A/B of the encoder in two library builds: semcode_amd/_lib/libsemcode_hip.so (new) against
# semcode_amd/_lib/libsemcode_hip_base.so (a build of the parent commit).  Three steps:
#   bits     the pooled outputs of small encoders of the three families, the diag_* results and every attention instantiation on its
#            own (scripts/ab_encoder.py dump / compare)
#   speed    the headline embed figure of bench.py three times per build, alternating, with its outputs dumped
#   kernels  the attention kernels' time per launch on the MiniLM and ModernBERT shapes, three times per build, alternating
# Every GPU step runs under its own time limit; the first failure ends the script.
#   bash scripts/ab_encoder.sh [OUT] [STEPS]      (defaults: build/ab_encoder, which git ignores; "bits speed kernels")  ->  OUT/report.log
set -o pipefail
OUT=${1:-build/ab_encoder}
STEPS=${2:-bits speed kernels}
L=semcode_amd/_lib
mkdir -p $OUT
: > $OUT/report.log
for step in $STEPS; do
    case $step in
    bits)
        timeout -k 10 300 python scripts/ab_encoder.py dump $L/libsemcode_hip_base.so $OUT/dump_base.txt || exit $?
        timeout -k 10 300 python scripts/ab_encoder.py dump $L/libsemcode_hip.so $OUT/dump_new.txt || exit $?
        python scripts/ab_encoder.py compare $OUT/dump_base.txt $OUT/dump_new.txt >> $OUT/report.log
        rc=$?
        tail -2 $OUT/report.log
        [ $rc = 0 ] || exit $rc
        ;;
    speed)
        rm -f $OUT/run_*.log
        i=0
        for v in base new base new base new; do
            i=$((i + 1))
            lib=$L/libsemcode_hip.so
            [ $v = base ] && lib=$L/libsemcode_hip_base.so
            timeout -k 10 180 python scripts/ab_encoder.py bench $lib --gpus 1 --steps 100 --warmup 10 --workload embed --dump-outputs $OUT/out_${i}_$v > $OUT/run_${i}_$v.log 2>&1
            rc=$?
            echo "== run $i $v rc=$rc"
            if [ $rc != 0 ]; then tail -20 $OUT/run_${i}_$v.log; exit $rc; fi
        done
        python scripts/ab_encoder.py speed $OUT | tee -a $OUT/report.log || exit $?
        ;;
    kernels)
        rm -f $OUT/attn_*.json
        i=0
        for v in base new base new base new; do
            i=$((i + 1))
            lib=$L/libsemcode_hip.so
            [ $v = base ] && lib=$L/libsemcode_hip_base.so
            timeout -k 10 240 python scripts/ab_encoder.py attn $lib $OUT/attn_${i}_$v.json || exit $?
        done
        python scripts/ab_encoder.py attnspeed $OUT | tee -a $OUT/report.log || exit $?
        ;;
    *) echo "unknown step $step"; exit 2 ;;
    esac
done
