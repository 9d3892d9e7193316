#!/bin/bash
# The measurement set a round ends with (one visit to a GPU machine): the whole GPU test suite with durations, the full bench under
# rocprofv3 --kernel-trace --stats, the FETCH / WRITE / busy PMC passes of the two attention launches (counters in their own runs) and the
# full bench as the driver runs it. usage: tools/round_end_runs.sh OUT_DIR (relative to the repository root); copy what is to be judged
# into profiles/.
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${1:?usage: tools/round_end_runs.sh OUT_DIR}
mkdir -p $R/$OUT
cd $R
(time timeout 1150 python -m pytest tests -x -q -m gpu --durations=15) > $OUT/pytest_gpu.log 2>&1
tail -3 $OUT/pytest_gpu.log
cd /tmp
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/prof -o bench -- python $R/bench.py --full --no-cpu-baseline --no-workloads --no-vae > $R/$OUT/bench_under_rocprof.log 2>&1
cd $R
tail -1 $OUT/bench_under_rocprof.log | cut -c1-300
timeout 300 bash tools/run_pmc_attn_traffic.sh $OUT/pmc_attn_traffic > $OUT/pmc_attn_traffic.log 2>&1
(time timeout 600 python bench.py --full --gpus 1 --steps 20 --warmup 5) > $OUT/bench_full.log 2>&1
tail -4 $OUT/bench_full.log | cut -c1-400
