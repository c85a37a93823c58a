#!/bin/bash
# one GPU call: default bench line, rocprof stats of the KD step and of the roofline leg, PMC passes; -> gpurun_out/
# usage (on the GPU box): bash tools/refresh_profiles.sh <tag>
TAG=${1:-r2b}
REPO=$(cd "$(dirname "$0")/.." && pwd)
cd "$REPO"
DEST=${DEST:-$REPO/bench_out}      # the full bench line and the KD-step profile's log
mkdir -p "$DEST"
python bench.py --full > "$DEST/bench_$TAG.json" 2> "$DEST/bench_$TAG.err"; echo "bench rc=$?"; tail -c 600 "$DEST/bench_$TAG.json"
bash tools/profile_bench.sh $TAG --full --no-secondary --no-cpu-baseline --steps 10 --warmup 4 > "$DEST/prof_$TAG.log" 2>&1; echo "prof rc=$?"
bash tools/profile_bench.sh ${TAG}_ko --kernel-only > gpurun_out/prof_${TAG}_ko.log 2>&1; echo "prof ko rc=$?"
bash tools/pmc_kernel_only.sh $TAG > gpurun_out/pmc_$TAG.log 2>&1; echo "pmc rc=$?"
rm -f gpurun_out/prof_$TAG/*kernel_trace.csv gpurun_out/prof_${TAG}_ko/*kernel_trace.csv gpurun_out/pmc_${TAG}_*/*kernel_trace.csv
du -sh gpurun_out | tail -1
