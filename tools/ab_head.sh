# A/B of the working tree's libpcx_hip.so against a build of the last commit (tools/_ab/libpcx_hip_head.so: `git worktree add /tmp/wt
# HEAD && make -C /tmp/wt/pothoscomms_amd/csrc && cp ...`), interleaved, long runs: tools/ab_head.sh [workloads...]
# AB_TREE_ENV="NAME=value ..." is put in front of the tree's runs (a switch of libpcx_hip_diag.so, with PCX_HIP_LIBRARY pointing at it).
# Every run has a time limit of its own, and the first one that does not end with status 0 ends the script: nothing more is started on
# a GPU that has just faulted or hung.
O=tools/_ab/libpcx_hip_head.so; WL=${@:-fir255 fmchain}
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
run() {
    local name=$1 w=$2; shift 2
    env "$@" timeout -k 10 150 python bench.py --no-cpu --workload $w --steps 1500 --warmup 300 > $T/line.json 2> $T/err.txt
    local rc=$?
    if [ $rc -ne 0 ]; then echo "$w $name: status $rc" >&2; tail -n 5 $T/err.txt >&2; exit $rc; fi
    python -c "import sys,json; d=json.loads(open('$T/line.json').read().strip().splitlines()[-1]); print('%-8s %-10s %.4f ms  frac %.4f' % ('$w', '$name', d['roofline']['avg_launch_ms'], d['roofline']['frac']))"
}
for rep in 1 2 3 4; do for w in $WL; do run head $w PCX_HIP_LIBRARY=$O; run tree $w ${AB_TREE_ENV:-PCX_AB=tree}; done; done
