# rocprofv3 kernel trace + tests/diag/timeline.py of one bench configuration:  bash tests/diag/timeline_run.sh <out dir> <name> [bench args]
mkdir -p $1; O=$(cd $1 && pwd); NAME=$2; shift 2
R=$PWD
cd /tmp && export TMPDIR=/tmp
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$NAME -o p -- python $R/bench.py --full --no-cpu-baseline --no-traffic --no-extras --steps 5 --warmup 3 "$@" > $O/bench_$NAME.json 2>/dev/null
cd $R
F=$(find $O/prof_$NAME -name "*kernel_trace.csv" | head -1)
python tests/diag/timeline.py $F > $O/timeline_$NAME.txt 2>&1
cp $(find $O/prof_$NAME -name "*kernel_stats.csv" | head -1) $O/stats_$NAME.csv
gzip -c $F > $O/trace_$NAME.csv.gz   # (a few MB: kept for offline analysis)
rm -rf $O/prof_$NAME
