#!/bin/bash
# usage: tools/prof.sh <workload> <outdir> <kernel-substring>   (on the GPU box; <outdir> relative to the repository root)
# kernel trace + PMC passes (counters in runs of their own, no tracing beside them).  Every pass runs under a time limit of its own and
# the script stops at the first pass that does not end with status 0: nothing more is started on a GPU that has just faulted or hung.
# PCX_HIP_LIBRARY in the environment profiles another build of the library (tools/_ab/libpcx_hip_head.so: the parent's).
W=$1; OUT=$2
export TMPDIR=/tmp
cd "$(dirname "$0")/.." || exit 1
rm -rf $OUT; mkdir -p $OUT
pass() {    # name, launches, rocprofv3 arguments...
    local name=$1 n=$2; shift 2
    timeout -k 10 180 rocprofv3 "$@" --output-format csv -d $OUT/$name -- python3 tools/prof_fir.py $W $n > $OUT/$name.log 2>&1
    local rc=$?
    if [ $rc -ne 0 ]; then echo "prof.sh: pass $name of $W ended with status $rc" >&2; tail -n 5 $OUT/$name.log >&2; exit $rc; fi
}
pass kt 5 --kernel-trace --stats
pass pmc1 3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY
pass pmc2 3 --pmc SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR
pass pmc3 3 --pmc FETCH_SIZE GRBM_GUI_ACTIVE
pass pmc4 3 --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum
python3 tools/prof_summary.py $OUT "$3" | tee $OUT/summary.txt
