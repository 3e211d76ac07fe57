set -e
OUT=${OUT:-prof_out}  # output directory, relative to the repository root
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt2 -o run -- python3 bench.py --full --steps 20 --no-cpu --strong-log 0 > $OUT/kt2.log 2>&1
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $OUT/valu2 -o run -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu --fri-log 0 --strong-log 0 > $OUT/valu2.log 2>&1
ls $OUT/kt2 $OUT/valu2
