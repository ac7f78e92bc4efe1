export PROFILE_TAG=r04_v2
LINES=${BENCH_LINES_DIR:-bench_out}; mkdir -p $LINES      # the bench lines (bench.py --full: every config on the line)
python bench.py --full --steps 20 --warmup 5 > $LINES/${PROFILE_TAG}_bench_t1124.json 2> $LINES/set_bench.err
python bench.py --full --proximal > $LINES/${PROFILE_TAG}_bench_t1124_prox.json 2>> $LINES/set_bench.err
python bench.py --full --workload s1500 > $LINES/${PROFILE_TAG}_bench_s1500.json 2>> $LINES/set_bench.err
python bench.py --full --workload s1500 --proximal > $LINES/${PROFILE_TAG}_bench_s1500_prox.json 2>> $LINES/set_bench.err
python bench.py --full --workload c5 > $LINES/${PROFILE_TAG}_bench_c5.json 2>> $LINES/set_bench.err
echo bench done
