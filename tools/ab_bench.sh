#!/bin/bash
# A/B (diagnostic): the headline bench with the default library against variant builds
# (variants/libragen_amd_NAME.so), one process per run, the libraries alternating: PAIRS rounds of
# plain `python bench.py`, then PAIRS rounds of `python bench.py --steps 20 --warmup 5`.  Every
# run's JSON line goes to OUT/ab_headline.jsonl with "lib" and "mode" added; us per rollout is
# printed as the runs finish.  Stops at the first run that fails.
#   tools/ab_bench.sh OUT NAME [NAME ...]      (PAIRS=6 by default)
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=gpurun_out/${1:-abbench}; shift; mkdir -p $OUT
PAIRS=${PAIRS:-6}
for mode in plain short; do
  if [ $mode = plain ]; then ARGS=""; else ARGS="--steps 20 --warmup 5"; fi
  for i in $(seq 1 $PAIRS); do
    for v in default "$@"; do
      if [ $v = default ]; then L=""; else L=$PWD/variants/libragen_amd_$v.so; fi
      RAGEN_AMD_LIB=$L timeout -k 10 240 python bench.py $ARGS > $OUT/run.json 2>> $OUT/err.log || exit 1
      python - "$OUT" "$v" "$mode" <<'EOF' | tee -a $OUT/ab.txt
import json, sys
out, lib, mode = sys.argv[1:4]
d = json.loads(open(out + "/run.json").read().strip().split("\n")[-1])
d["lib"], d["mode"] = lib, mode
open(out + "/ab_headline.jsonl", "a").write(json.dumps(d) + "\n")
print(lib, mode, round(d["ms_per_step"] * 1e3, 3))
EOF
    done
  done
done
python - "$OUT" <<'EOF' | tee -a $OUT/ab.txt
import json, statistics, sys
rows = [json.loads(l) for l in open(sys.argv[1] + "/ab_headline.jsonl")]
for mode in ("plain", "short"):
    for lib in sorted({r["lib"] for r in rows}):
        x = [r["ms_per_step"] * 1e3 for r in rows if r["lib"] == lib and r["mode"] == mode]
        if x:
            print(f"{mode:6} {lib:10} n={len(x)} median {statistics.median(x):.3f} min {min(x):.3f} max {max(x):.3f} us")
EOF
