#!/bin/bash
# round 6: the whole GPU suite + the --full bench line (tag in $1), written under $OUT_DIR (default runs/)
tag=${1:-r06x}
O=${OUT_DIR:-runs}
mkdir -p "$O"
( time python -m pytest tests -x -q -m gpu -p no:cacheprovider ) > "$O/${tag}_gpu_tests.log" 2>&1
tail -4 "$O/${tag}_gpu_tests.log" | cut -c1-600
python bench.py --full --detail "$O/${tag}_bench_detail.json" > "$O/${tag}_bench.line" 2> "$O/${tag}_bench.err"
tail -c 3000 "$O/${tag}_bench.line"
