# round 5, GPU call 1: the hybrid build -- parity (unchained), smoke, default bench line, kernel stats / timeline:  bash tests/diag/r05_hybrid_first.sh <out dir>
O=$1; mkdir -p $O
(timeout 900 python -m pytest tests/test_e2e_unchained_gpu.py tests/test_fulldepth_parity_gpu.py::test_full_depth_hybrid_precision_unchained -q -x -s --timeout 600 2>&1 | grep -v "^$" | tail -80 > $O/hybrid_tests.log)
(timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1)
t0=$(date +%s)
(timeout 700 python bench.py --full --gemm-breakdown $O/gemm_shapes_b14.txt > $O/bench.json 2> $O/bench.err)
echo "wall seconds: $(( $(date +%s) - t0 ))" > $O/bench_wall.txt
bash tests/diag/timeline_run.sh $O hybrid
bash tests/diag/timeline_run.sh $O bf16vit --vit-operands same
tail -3 $O/hybrid_tests.log; tail -3 $O/smoke.log; head -c 600 $O/bench.json; echo; cat $O/bench_wall.txt; head -30 $O/timeline_hybrid.txt
