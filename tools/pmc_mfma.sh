#!/bin/bash
# GPU box: one SQ PMC pass over the C4 bench (MFMA utilisation of the BA kernels); results in $OUT
# (default: prof_out/ under the repository)
R=${GRAFT_REPO_ROOT:-$(pwd)}; cd /tmp && export TMPDIR=/tmp && cd "$R" || exit 1
O=${OUT:-prof_out}
mkdir -p $O && rm -rf $O/pmcmf
timeout -s KILL 90 rocprofv3 --pmc SQ_INSTS_VALU_MFMA_MOPS_F64 SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU SQ_BUSY_CYCLES SQ_WAVES \
  -d $O/pmcmf -o mf --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/pmcmf.log 2>&1
