# usage: bash tools/run_bench_prof.sh TAG  -- bench line + rocprofv3 kernel stats of the bench
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}  # output directory, relative to the repository root
mkdir -p $OUT
TAG=$1
timeout -k 10 300 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { tail -20 $OUT/${TAG}_bench.err; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_kt -o run -- python3 bench.py --full --steps 20 --no-cpu > $OUT/${TAG}_kt.log 2>&1
echo done
