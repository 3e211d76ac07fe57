# N = 2 rehearsal of the driver's multi-GPU bench on a one-GPU box: both ranks
# share cuda:0 and exchange through gloo (the script's logic, not a result).
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-prof_out}  # output directory, relative to the repository root
mkdir -p $OUT
export MLH_BENCH_BACKEND=gloo
timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --full --steps 5 --warmup 2 --no-cpu > $OUT/n2_bench.json 2> $OUT/n2_bench.err || { tail -30 $OUT/n2_bench.err; exit 1; }
cat $OUT/n2_bench.json
