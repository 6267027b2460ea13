#!/bin/bash
# The one GPU-box runner (replaces the per-experiment r3_*.sh scripts).  From the repo root on the GPU box:
#
#   gpurun --timeout 1500 -- 'bash tools/gpu_round.sh <tag> [tests] [bench] [prof] [kbench "<kbench args>"]'
#
# Results go to $OUT_ROOT/<tag>/ (OUT_ROOT defaults to out, which git ignores):
#   tests   python -m pytest tests -m gpu -x -q                          -> tests.log
#   ktests "<expr>"   the same with -k <expr>                            -> ktests.log
#   bench   python bench.py --full --steps 20 --warmup 5                 -> bench.json (every record, not only the headline)
#   benchlive  the same with --live-traffic (roofline.traffic collected by the run itself)  -> bench_live.json
#   prof    tools/prof_bench.sh <tag> (rocprofv3 --kernel-trace --stats, default + one-stream; FETCH_SIZE / WRITE_SIZE passes)
#   kbench  python tools/kbench.py <args> (single-kernel timings)        -> kbench.log
#
# Counter passes for single kernels: tools/pmc.sh, tools/pmc_lds.sh, tools/pmc_mfma.sh, tools/pmc_one.sh (each documents itself).
# Copy what is to be judged from $OUT_ROOT/<tag>/ into profiles/ (tracked) afterwards.
set -u
TAG=$1; shift
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
O=${OUT_ROOT:-out}/$TAG
mkdir -p $O
while [ $# -gt 0 ]; do
  case $1 in
    tests)  timeout 1500 python -m pytest tests -m gpu -q --tb=short -rs 2>&1 | grep -v "curr_density\|amdgpu.ids" | tail -150 > $O/tests.log ;;
    ktests) shift; timeout 1500 python -m pytest tests -m gpu -x -q --tb=short -k "$1" 2>&1 | grep -v "curr_density\|amdgpu.ids" | tail -150 > $O/ktests.log ;;
    bench)  timeout 900 python bench.py --full --steps 20 --warmup 5 > $O/bench.json 2> $O/bench.err ;;
    benchlive) timeout 1500 python bench.py --full --steps 20 --warmup 5 --live-traffic > $O/bench_live.json 2> $O/bench_live.err ;;
    prof)   bash tools/prof_bench.sh $TAG 2>&1 | tail -20 > $O/prof.log ;;
    kbench) shift; timeout 600 python tools/kbench.py $1 > $O/kbench.log 2>&1 ;;
  esac
  shift
done
tail -5 $O/*.log 2>/dev/null
