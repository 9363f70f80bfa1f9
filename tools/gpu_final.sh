#!/bin/bash
# usage (GPU box): bash tools/gpu_final.sh <tag>  -> the suite's log next to prof_<tag>/ and pmc_<tag>/ (where tools/gpu_prof.sh
#   and tools/gpu_pmc.sh put them); the bench lines in $OUT/bench_<tag>/ (OUT defaults to out/ in the repository)
# The round's closing artefacts of one build: the full GPU test suite, the kernel-trace profile + PMC passes of the headline
# config, the four bench lines (--full: every leg; base and large with --live-traffic, sat_large, extract) and the Large
# kernel-trace summary; copy what is to be judged into profiles/rNN/.
TAG=${1:-x}
cd $GRAFT_REPO_ROOT; mkdir -p gpurun_out; export TMPDIR=/tmp
timeout 1500 python -m pytest tests -q -m gpu > gpurun_out/pytest_gpu_$TAG.txt 2>&1; tail -3 gpurun_out/pytest_gpu_$TAG.txt
timeout 600 bash tools/gpu_prof.sh $TAG
timeout 900 bash tools/gpu_pmc.sh $TAG                      # base: FETCH / WRITE / SQ passes -> pmc_<tag>/gemm_hbm_traffic_base.json
CFG=large SQ=0 timeout 600 bash tools/gpu_pmc.sh ${TAG}_large   # large: traffic passes only -> pmc_<tag>_large/gemm_hbm_traffic_large.json
B=${OUT:-out}/bench_$TAG; mkdir -p "$B"
timeout 600 python bench.py --steps 20 --warmup 5 --full --live-traffic --no-secondary > "$B/base.txt" 2>&1; tail -1 "$B/base.txt" | cut -c1-260
timeout 600 python bench.py --config large --steps 10 --warmup 3 --full --live-traffic > "$B/large.txt" 2>&1; tail -1 "$B/large.txt" | cut -c1-260
for c in sat_large extract; do timeout 400 python bench.py --config $c --steps 10 --warmup 3 --full > "$B/$c.txt" 2>&1; tail -1 "$B/$c.txt" | cut -c1-260; done
CFG=large timeout 400 bash tools/gpu_prof_large.sh; cp gpurun_out/prof_large/summary.txt gpurun_out/summary_large_$TAG.txt 2>/dev/null
(for c in large sat_large extract; do tail -1 "$B/$c.txt"; done) > "$B/lines.jsonl"
