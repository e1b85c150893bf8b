#!/bin/bash
# BASELINE configs[3] (C4) under rocprofv3: kernel trace + stats, then FETCH_SIZE / WRITE_SIZE passes (one run each),
# converted to bytes with tools/pmc_calib's factors (run tools/step_pmc.sh first, with the same $STEP_PMC_OUT: it
# leaves the calibration passes in $O/calib_pmc_*).  Writes $O/c4_kernel_stats.csv and $O/c4_pmc.json ->
# profiles/r<round>_c4_*  (O = $STEP_PMC_OUT, default profile_out, as tools/step_pmc.sh).
set -e
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
O=${STEP_PMC_OUT:-profile_out}
mkdir -p $O
rocprofv3 --kernel-trace --stats --output-format csv -d $O/c4_trace -o p -- python3 tools/pmc_run_c4.py > $O/c4_trace.log 2>&1
grep -E '^"Name"|step_|edt_|pack_bitmap|path_' $O/c4_trace/p_kernel_stats.csv > $O/c4_kernel_stats.csv
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --output-format csv --pmc $c -d $O/c4_pmc_$c -o p -- python3 tools/pmc_run_c4.py > $O/c4_pmc_$c.log 2>&1
done
python3 tools/pmc_summary.py c4 $O/c4_pmc_ $O/calib_pmc_ $O/c4_pmc.json 65536 $((4183 * 65536))
cat $O/c4_kernel_stats.csv
