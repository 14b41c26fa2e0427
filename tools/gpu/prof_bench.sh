set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
OUT=${OUT:?set OUT to the folder the results go to}
mkdir -p $OUT/pb
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $OUT/pb/bench.json 2> $OUT/pb/bench.err || exit 1
cat $OUT/pb/bench.json | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['roofline']['avg_launch_ms'], d['fullsort']['kernel_ms_all_eval_users'])"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/pb/prof -o b -- python bench.py --full --no-cpu-baseline > $OUT/pb/benchp.json 2> $OUT/pb/benchp.err || exit 1
f=$(find $OUT/pb/prof -name '*kernel_stats.csv' | head -1); cut -d, -f1-4 "$f" | head -14
find $OUT/pb/prof -name '*kernel_trace.csv' -delete
