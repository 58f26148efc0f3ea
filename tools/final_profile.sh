#!/bin/bash
# usage (MI355X, repo root): tools/final_profile.sh <tag> [output dir, default profile_out]  -> <output dir>/<tag>_*: gpu tests, --full bench line,
# the same bench under rocprofv3 --kernel-trace --stats, the hard-data config (collect pass)
tag=$1
out=${2:-profile_out}
mkdir -p $out
export TMPDIR=/tmp
python -m pytest tests -m gpu -x -q > $out/${tag}_tests.log 2>&1 || { tail -30 $out/${tag}_tests.log; exit 1; }
tail -1 $out/${tag}_tests.log
python bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err || exit 1
rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_prof -- python3 bench.py --full --no-cpu-baseline --no-gemm-ref --steps 10 > $out/${tag}_bench_prof.json 2> $out/${tag}_prof.err || exit 1
python bench_configs.py --mode hard > $out/${tag}_cfg_hard.json 2> $out/${tag}_cfg_hard.err || exit 1
find $out/${tag}_prof -name "*kernel_stats.csv"
