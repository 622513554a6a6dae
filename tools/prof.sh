#!/bin/bash
# usage (on the GPU box, from the repo root): tools/prof.sh <tag> <bench args...>
# rocprofv3 --kernel-trace --stats of `python bench.py <args>`; summary -> $GM_TOOLS_OUT/<tag>_kernel_stats.txt (default tools_out/)
tag=$1; shift
root=${GRAFT_REPO_ROOT:-$(pwd)}
outdir=$(cd $root && mkdir -p ${GM_TOOLS_OUT:-tools_out} && cd ${GM_TOOLS_OUT:-tools_out} && pwd)
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof_$tag
rocprofv3 --kernel-trace --stats -d /tmp/prof_$tag -o p -- python $root/bench.py "$@" > $outdir/${tag}_profiled_bench.json 2> /tmp/prof_$tag.err
db=$(find /tmp/prof_$tag -name "*.db" | head -1)
python $root/tools/rocprof_summary.py $db $outdir/${tag}_kernel_stats.txt > /dev/null
head -${PROF_LINES:-25} $outdir/${tag}_kernel_stats.txt
