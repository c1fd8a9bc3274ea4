# usage: bash tools/prof_step.sh <version tag>; writes the bench line under rocprofv3 and the steady-state kernel summary to
# $PROF_OUT (default prof_out/). --full: the last 8 steps of the trace are the optimizer-less steps of `fwd_bwd_only`.
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
V=$1
OUT=${PROF_OUT:-prof_out}
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof -o sec -- python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --scoring-pool 0 --pvrcnn-steps 0 --bf16x3-steps 0 --miopen-steps 0 > "$OUT/${R:-r06}_bench_under_rocprof_$V.json" 2>"$OUT/prof_err.log"
PROF_LIST=chain_,table_rows,tables_,hash_build,fillBuffer,vox_,nbr_permute PROF_SPLIT_GRID=sparse_conv_fwd2 PROF_GAPS=12 python tools/prof_summary.py $(find /tmp/prof -name "*kernel_trace.csv" | head -1) 8 > "$OUT/${R:-r06}_second_bs16_steady_state_kernel_summary_$V.csv"
head -1 "$OUT/${R:-r06}_second_bs16_steady_state_kernel_summary_$V.csv"
