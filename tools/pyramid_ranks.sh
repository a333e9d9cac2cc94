O=${1:?usage: bash tools/pyramid_ranks.sh OUTDIR}
mkdir -p $O
set -e
python bench.py --full --workload pyramid > $O/pyr_n1.json 2> $O/pyr_n1.err
timeout -k 10 500 python bench.py --full --gpus 2 --rehearse-one-gpu --workload pyramid --steps 2 --warmup 1 > $O/pyr_n2.json 2> $O/pyr_n2.err
