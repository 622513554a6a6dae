#!/bin/bash
cd ${GRAFT_REPO_ROOT:-.}
outdir=${GM_TOOLS_OUT:-tools_out}; mkdir -p $outdir
python bench.py --full --steps 100 --warmup 10 --repeats 2 --no-cpu-baseline --no-fwd-bwd > $outdir/fwd_$1.json 2> $outdir/fwd_$1.err || tail -3 $outdir/fwd_$1.err
python tools/show.py $outdir/fwd_$1.json
