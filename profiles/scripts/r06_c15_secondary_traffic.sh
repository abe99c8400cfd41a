# round 6, call 15: counter bytes for secondary rows (the harness's --mode bwd / nhwc), then the --full bench line
OUT=${1:?usage: $0 OUTDIR}; mkdir -p $OUT
(tools/sweep_bench --workload nstar --mode bwd --rounds 3 --launches 2; tools/sweep_bench --workload kitti --mode bwd --rounds 3 --launches 3; tools/sweep_bench --workload kitti --mode nhwc --rounds 3 --launches 3) > $OUT/harness_modes.txt 2>&1
python bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
