# usage: prof.sh TAG [extra env assignments are exported by the caller]
# writes TAG_prof_bench.json, TAG_last_step.txt and TAG_kernel_stats.csv to $OUT (default: prof_out/ in the repository root)
TAG=$1
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/prof_out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o $TAG -- python3 $ROOT/bench.py --steps 2 --warmup 1 --full --no-cpu-baseline --radiation-freq 0 --no-class-layer $BENCH_EXTRA > $OUT/${TAG}_prof_bench.json 2> $OUT/${TAG}_prof.err
cd $ROOT
f=$(find $OUT/${TAG}_prof -name "*kernel_trace.csv" | head -1)
python scripts/step_breakdown.py $f > $OUT/${TAG}_last_step.txt
s=$(find $OUT/${TAG}_prof -name "*kernel_stats.csv" | head -1)
cp $s $OUT/${TAG}_kernel_stats.csv
rm -rf $OUT/${TAG}_prof
