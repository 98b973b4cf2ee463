#!/bin/bash
# several builds side by side on ONE box (each a directory with bench.py + erasor_amd/ like _ab_old/): the driver's statistic and 100-step
# passes, the directories in rotation, AB_REPS times (default 2).   tools/ab_dirs.sh <dir> <dir> ...   (AB_WORKLOADS as in tools/ab_old_new.sh)
# A run that fails or runs out of time ends the whole call: nothing more is started on a device that may have faulted.
set -o pipefail
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
A="--no-cpu-baseline --no-extra-workloads --no-callback-bench --no-pr-rr"
run() { timeout -k 10 300 python $1/bench.py $A $2 2>/dev/null | python -c "
import json,sys; d=json.loads(sys.stdin.read().strip().split(chr(10))[-1]); print('%-10s' % '$1', d['ms_per_step'], d['ms_per_step_all'][:3], 'auto', [round(x,1) for x in (d['overlapped_steps']['auto']['plain_period_us'], d['overlapped_steps']['auto']['overlapped_period_us'])])"; }
for wl in ${AB_WORKLOADS:-"--workload=seq05" "--workload=large_scale_05"}; do
  for cfg in "--steps 20 --warmup 5 --repeats 7" "--steps 100 --warmup 5 --repeats 5"; do
    echo "== $wl $cfg"
    for rep in $(seq ${AB_REPS:-2}); do for d in "$@"; do run $d "$wl $cfg" || { echo "run failed ($d $wl $cfg): stopping"; exit 1; }; done; done
  done
done
