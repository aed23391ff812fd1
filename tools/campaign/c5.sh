set -o pipefail
OUT=${1:?usage: tools/campaign/c5.sh OUTPUT_DIR}
mkdir -p $OUT
export HSA_ENABLE_IPC_MODE_LEGACY=0
timeout -k 10 240 python -m torch.distributed.run --nnodes=1 --nproc-per-node 4 --master-addr 127.0.0.1 --master-port 29611 bench.py --full --gpus 4 --share-gpu --no-class-surface > $OUT/r06_bench_survey3_65536_4ranks_share_gpu.json 2> $OUT/share4.err; echo "share4 rc=$?"
timeout -k 10 200 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29612 bench.py --full --gpus 2 --share-gpu --no-class-surface > $OUT/r06_bench_survey3_65536_2ranks_share_gpu.json 2> $OUT/share2.err; echo "share2 rc=$?"
timeout -k 10 200 python bench.py --full --force-dist --no-class-surface > $OUT/r06_bench_survey3_65536_force_dist.json 2> $OUT/force.err; echo "force rc=$?"
timeout -k 10 200 python bench.py --full --node 2 --share-gpu --no-class-surface > $OUT/r06_bench_survey3_65536_node2_share_gpu.json 2> $OUT/node2.err; echo "node2 rc=$?"
timeout -k 10 300 python bench.py --full --workload corpus --corpus-streams 600 --no-class-surface > $OUT/r06_bench_corpus_600.json 2> $OUT/corpus600.err; echo "corpus600 rc=$?"
