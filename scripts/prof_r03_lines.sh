# Round-3 lines beside the headline: netf, C5 (all 8 row-interleaved shards on one GPU), occlusion with
# path C's AABB selection (batched step), AABB selection without occlusion
set -o pipefail
OUT=gpurun_out/prof_c3_netf PASSES="bench kt" bash scripts/prof_c3.sh --mode netf --steps 5 --warmup 2 || exit 1
C5=${C5_OUT:-out/c5}    # where the C5 line goes
mkdir -p $C5 && NLOSGR_BENCH_PROGRESS=1 timeout -k 10 600 python bench.py --full --config C5 --band 8 --steps 3 --warmup 1 --no-cpu-baseline > $C5/bench_band8.log 2> $C5/bench_band8.err || exit 1
tail -1 $C5/bench_band8.log | cut -c1-300
OUT=gpurun_out/prof_c3_occl_aabb PASSES="bench kt" bash scripts/prof_c3.sh --mode occl --selection aabb --steps 3 --warmup 1 --no-cpu-baseline || exit 1
