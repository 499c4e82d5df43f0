#!/usr/bin/env bash
# One gpurun call: GPU tests, the bench lines of every workload, and (optionally) the rocprofv3 evidence.
#   bash tools/gpu_round.sh <tag> [profile workloads...]
export RESULTS=${RESULTS:-results}   # output root; profiles/collect.sh writes its prof_<tag>/ under the same root
TAG=${1:-run}; shift || true
mkdir -p $RESULTS/$TAG
python3 -m pytest tests -x -q -m gpu > $RESULTS/$TAG/pytest_gpu.log 2>&1; echo "pytest rc=$?" | tee -a $RESULTS/$TAG/pytest_gpu.log
tail -3 $RESULTS/$TAG/pytest_gpu.log
for wl in c2 c3 c4 c5; do
    python3 bench.py --full --workload $wl $( [ $wl != c2 ] && echo --no-cpu-baseline ) > $RESULTS/$TAG/bench_$wl.json 2> $RESULTS/$TAG/bench_$wl.err
    python3 - $RESULTS/$TAG/bench_$wl.json <<'PY'
import json, sys
try:
    j = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
    print(j["config"]["workload"][:50], "ms/step %.3f" % j["ms_per_step"], {k: round(v["ms"], 4) for k, v in j["kernels"].items()}, "frac %.3f" % j["roofline"]["frac"])
except Exception as e:
    print("bench failed", sys.argv[1], e)
PY
done
for wl in "$@"; do
    bash profiles/collect.sh $wl --workload $wl > $RESULTS/$TAG/collect_$wl.log 2>&1
    mkdir -p $RESULTS/$TAG/prof_$wl
    cp $RESULTS/prof_$wl/summary.txt $RESULTS/prof_$wl/traffic.json $RESULTS/$TAG/prof_$wl/ 2>/dev/null
done
