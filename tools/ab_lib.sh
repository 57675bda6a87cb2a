#!/bin/bash
# A/B of two built libraries in ONE GPU call: [AB_REPS=n] tools/ab_lib.sh libA.so libB.so [bench args]   (paths under change3d_amd/lib/)
# The runs alternate A, B, A, B, ... (AB_REPS of each, default 2).  A run that fails ends the script: nothing more is started on
# a GPU that may have faulted.
set -u -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
mkdir -p gpurun_out
A=$1; B=$2; shift 2
for rep in $(seq 1 "${AB_REPS:-2}"); do
  for L in $A $B; do
    C3D_LIB=$(pwd)/change3d_amd/lib/$L timeout -k 10 600 python bench.py --steps 30 --warmup 5 --no-cpu-baseline --no-also --no-kernel-profile "$@" 2>/dev/null | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('$L rep $rep', d['ms_per_step'], 'ms', d['value'], 'img/s')" || exit 1
  done
done
