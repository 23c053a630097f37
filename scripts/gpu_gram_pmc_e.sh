#!/bin/bash
# SQ counters + GRBM_GUI_ACTIVE (the clock) of the wide Gram kernel k_gram3e on
# probe_gram.py (N = 10k, random rows), at two depths. One rocprofv3 --pmc pass per depth.
set -o pipefail
out=gpurun_out/${1:-gram_pmc_e}
mkdir -p $out
export TMPDIR=/tmp REPS=2
C="SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS SQ_INST_CYCLES_VMEM GRBM_GUI_ACTIVE"
for ds in 43264 290400; do
  DS=$ds timeout -s KILL 120 rocprofv3 --pmc $C -d $out/e$ds -o p --output-format csv \
      -- python scripts/probe_gram.py > $out/e$ds.log 2>&1 || { echo "pmc $ds failed"; tail -5 $out/e$ds.log; exit 1; }
  python3 scripts/gram_pmc_summary.py $out/e$ds/p_counter_collection.csv e $ds
done
