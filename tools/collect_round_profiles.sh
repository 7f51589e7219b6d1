# Round profiles: steady-state kernel summary of the training step, per-(kernel, grid) totals, layer kernel summaries, final bench lines.
# usage (GPU box): bash tools/collect_round_profiles.sh r03 OUTDIR
R=${1:-rXX}
OUT=${2:?usage: collect_round_profiles.sh TAG OUTDIR}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace -d $OUT/prof_step -o step --output-format csv -- python3 bench.py --steps 12 --warmup 4 > $OUT/${R}_prof_step.json 2> $OUT/${R}_prof_step.err
F=$(ls $OUT/prof_step/*kernel_trace.csv $OUT/prof_step/*/*kernel_trace.csv 2>/dev/null | head -1)
python3 tools/summarize_trace.py $F --skip 2 --top 80 > $OUT/${R}_bench_step_steady_kernel_stats.csv
python3 tools/summarize_by_grid.py $F --skip 2 --match ipsr > $OUT/${R}_own_kernels_by_grid.txt
rm -rf $OUT/prof_step
for cfg in "2:1" "4:3"; do
  c=${cfg%%:*}; p=${cfg#*:}
  rocprofv3 --kernel-trace --stats -d $OUT/prof_layer -o layer --output-format csv -- python3 tools/profile_layer.py --cfg $c --patch $p > $OUT/${R}_layer_cfg${c}_p${p}.txt 2>&1
  S=$(ls $OUT/prof_layer/*kernel_stats.csv $OUT/prof_layer/*/*kernel_stats.csv 2>/dev/null | head -1)
  head -30 $S > $OUT/${R}_layer_cfg${c}_p${p}_kernel_stats.csv
  rm -rf $OUT/prof_layer
done
python3 bench.py --full --steps 20 > $OUT/${R}_bench_final.json 2> $OUT/${R}_bench_final.err
python3 bench.py --full --steps 20 --dtype bf16 --batch 16 --no-cpu-baseline > $OUT/${R}_bench_bf16.json 2> $OUT/${R}_bench_bf16.err
# HBM traffic of the layer's kernels (two PMC passes, no other tracing) -> ${R}_layer_cfg2_hbm_traffic.csv and profiles/traffic_corr_argmax.json
for pass in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $pass -d $OUT/pmc_layer_$pass -o l --output-format csv -- python3 tools/profile_layer.py --cfg 2 --iters 3 > $OUT/pmc_layer_$pass.log 2>&1
done
FF=$(ls $OUT/pmc_layer_FETCH_SIZE/*counter_collection.csv $OUT/pmc_layer_FETCH_SIZE/*/*counter_collection.csv 2>/dev/null | head -1)
FW=$(ls $OUT/pmc_layer_WRITE_SIZE/*counter_collection.csv $OUT/pmc_layer_WRITE_SIZE/*/*counter_collection.csv 2>/dev/null | head -1)
python3 tools/collect_traffic.py $FF $FW > $OUT/${R}_layer_cfg2_hbm_traffic.csv && cp profiles/traffic_corr_argmax.json $OUT/${R}_traffic_corr_argmax.json
rm -rf $OUT/pmc_layer_FETCH_SIZE $OUT/pmc_layer_WRITE_SIZE
python3 tools/engine_map.py > $OUT/${R}_engine_map.txt 2> $OUT/${R}_engine_map.err
