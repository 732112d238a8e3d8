# Round-end measurement on the GPU box: the full -m gpu suite, smoke(), the driver-form bench line (+ extras), rocprofv3 kernel
# stats / timelines of the forward and the generate step, per-shape GEMM tables at 14 / 4 / 1 images per call, serving throughput.
# Everything lands under <out dir>; the summaries worth keeping are copied into profiles/ by hand.   bash tests/diag/round_end_measure.sh <out dir>
mkdir -p $1; O=$(cd $1 && pwd)
(timeout 1300 python -m pytest tests -q -m gpu --timeout 600 2>&1 | tail -60 > $O/gpu_tests.log)
(timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1)
(timeout 700 python bench.py --full --gemm-breakdown $O/gemm_shapes_b14.txt > $O/bench.json 2> $O/bench.err)
(timeout 200 python bench.py --batch 4 --steps 10 --warmup 3 --full --no-cpu-baseline --no-traffic --no-extras --gemm-breakdown $O/gemm_shapes_b4.txt > $O/bench_b4.json 2>/dev/null)
(timeout 200 python bench.py --batch 1 --steps 10 --warmup 3 --full --no-cpu-baseline --no-traffic --no-extras --gemm-breakdown $O/gemm_shapes_b1.txt > $O/bench_b1.json 2>/dev/null)
(timeout 300 python tests/serve_bench.py > $O/serve_bench.txt 2>&1)
R=$PWD
cd /tmp && export TMPDIR=/tmp
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_fwd -o fwd -- python $R/bench.py --full --no-cpu-baseline --no-traffic --no-extras --steps 5 --warmup 3 > $O/bench_prof.json 2>/dev/null
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_gen -o gen -- python $R/bench.py --full --mode generate --batch 4 --steps 2 --warmup 2 --no-cpu-baseline --no-traffic > $O/bench_gen_prof.json 2>/dev/null
cd $R
F=$(find $O/prof_fwd -name "*kernel_trace.csv" | head -1); G=$(find $O/prof_gen -name "*kernel_trace.csv" | head -1)
python tests/diag/timeline.py $F > $O/timeline_b14.txt 2>&1
python tests/diag/decode_trace.py $G > $O/decode_step.txt 2>&1
cp $(find $O/prof_fwd -name "*kernel_stats.csv" | head -1) $O/fwd_kernel_stats.csv
cp $(find $O/prof_gen -name "*kernel_stats.csv" | head -1) $O/gen_kernel_stats.csv
rm -rf $O/prof_fwd $O/prof_gen
grep -n "passed\|failed" $O/gpu_tests.log | tail -2; tail -2 $O/smoke.log; head -c 200 $O/bench.json; echo; cat $O/serve_bench.txt | tail -3; tail -2 $O/decode_step.txt
