#!/usr/bin/env bash
# Round 5: rocprofv3 evidence (kernel trace + FETCH / WRITE counters) and a bench line per workload (GPU box, through gpurun):
#   bash tools/r5_profiles.sh wl1 wl2 ...        ("c3:1" = workload c3 with --pad 1)
# -> $RESULTS/r5p/r05_<tag>_{rocprof_summary.txt,traffic.json,bench.json}; copy what should be judged into profiles/.
export RESULTS=${RESULTS:-results}   # output root; profiles/collect.sh writes its prof_<tag>/ under the same root
mkdir -p $RESULTS/r5p
for spec in "$@"; do
    wl=${spec%%:*}; pad=0; tag=$wl
    if [[ "$spec" == *:* ]]; then pad=${spec##*:}; tag=${wl}_pad$pad; fi
    bash profiles/collect.sh $tag --workload $wl --pad $pad > $RESULTS/r5p/collect_$tag.log 2>&1
    cp $RESULTS/prof_$tag/summary.txt $RESULTS/r5p/r05_${tag}_rocprof_summary.txt 2>/dev/null
    cp $RESULTS/prof_$tag/traffic.json $RESULTS/r5p/r05_${tag}_traffic.json 2>/dev/null
    python3 bench.py --full --workload $wl --pad $pad --no-cpu-baseline --no-configs > $RESULTS/r5p/r05_${tag}_bench.json 2> $RESULTS/r5p/bench_$tag.err
    python3 - $RESULTS/r5p/r05_${tag}_bench.json $tag <<'PY'
import json, sys
try:
    j = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
    print("%-10s ms/step %.4f  %s" % (sys.argv[2], j["ms_per_step"], "  ".join("%s %.4f ms %.2f (box %s)" % (k, v["ms"], v["GB/s"] / 8000, ("%.2f" % v["frac_of_box"]) if "frac_of_box" in v else "-") for k, v in j["kernels"].items())))
except Exception as e:
    print("bench failed", sys.argv[2], e)
PY
    rm -rf $RESULTS/prof_$tag
done
