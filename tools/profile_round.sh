# Round profile set (run on the GPU box from the repo root):
#  kernel stats of the bench, separate FETCH_SIZE / WRITE_SIZE passes, and a
#  VALU-counter pass with kernel trace.  Summaries: tools/pmc_summary.py and
#  tools/valu_summary.py (run afterwards on the output directory).
set -e
OUT=${OUT:-prof_out}  # output directory, relative to the repository root
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt -o run -- python3 bench.py --full --steps 20 --no-cpu > $OUT/kt.log 2>&1
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/fetch -o run -- python3 bench.py --steps 5 --warmup 1 --no-cpu --no-extras > $OUT/fetch.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/write -o run -- python3 bench.py --steps 5 --warmup 1 --no-cpu --no-extras > $OUT/write.log 2>&1
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $OUT/valu -o run -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu --fri-log 0 > $OUT/valu.log 2>&1
find $OUT -name "*.csv" | head -20
