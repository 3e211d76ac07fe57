set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}  # output directory, relative to the repository root
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/${1:-r02u}_gputest.log 2>&1 || { tail -30 $OUT/${1:-r02u}_gputest.log; exit 1; }
tail -2 $OUT/${1:-r02u}_gputest.log
timeout -k 10 300 python bench.py --full > $OUT/${1:-r02u}_bench.json 2> $OUT/${1:-r02u}_bench.err || { tail -20 $OUT/${1:-r02u}_bench.err; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${1:-r02u}_kt -o run -- python3 bench.py --full --steps 20 --no-cpu > $OUT/${1:-r02u}_kt.log 2>&1
echo done
