#!/bin/bash
# Everything profiles/rNN_* is made from, in one run on the GPU box:  OUT=<results folder> bash tools/record_round.sh r03
# (kernel stats + PMC passes of the default command, VALU counters, the batch profile, one --full bench line per workload)
# afterwards: python tools/summarize_batch_profile.py r03; copy profile_round.sh's {summary.json,kernel_stats.csv} and $OUT/r03_*.json to profiles/
tag=${1:-r03}
R=$GRAFT_REPO_ROOT
O=${OUT:?set OUT to the folder the results are written to}
cd $R
mkdir -p $O
bash tools/profile_round.sh $tag > $O/${tag}_profile_round.log 2>&1
bash tools/pmc_valu.sh $tag > $O/${tag}_pmc_valu.log 2>&1
bash tools/profile_batch.sh > $O/${tag}_profile_batch.log 2>&1
cd $R
python3 bench.py --full > $O/${tag}_bench_default.json 2> $O/${tag}_bench_default.err
python3 bench.py --full --workload large > $O/${tag}_bench_large.json 2>/dev/null
python3 bench.py --full --workload large --near-guess > $O/${tag}_bench_large_near.json 2>/dev/null
python3 bench.py --full --workload large --extent 200 > $O/${tag}_bench_large200.json 2>/dev/null
python3 bench.py --full --workload batch --batch 64 > $O/${tag}_bench_batch64.json 2>/dev/null
python3 bench.py --full --workload batch --batch 256 > $O/${tag}_bench_batch256.json 2>/dev/null
python3 bench.py --full --workload mapbuild > $O/${tag}_bench_mapbuild_n1.json 2>/dev/null
python3 bench.py --full --workload pyramid > $O/${tag}_bench_pyramid.json 2>/dev/null
python3 tools/time_pair.py 2>/dev/null | tail -1 > $O/${tag}_pair_sequence.json
python3 tools/node_loop_profile.py 40 60000 node $O/${tag}_node_loop.json > $O/${tag}_node_loop.log 2>&1
python3 tools/node_loop_profile.py 40 60000 rosbag $O/${tag}_node_loop_rosbag.json > $O/${tag}_node_loop_rosbag.log 2>&1
bash tools/pmc_valu_split.sh $tag > $O/${tag}_pmc_valu_split.log 2>&1
python3 tools/time_k1_forms.py > $O/${tag}_k1_forms.jsonl 2>/dev/null
python3 tools/time_prefilter.py 2>/dev/null | tail -1 > $O/${tag}_prefilter.json
ls -la $O/${tag}_*.json
