#!/bin/bash
# same-box A/B of environment settings on the working tree: tools/ab_env.sh <tag> <rounds> "<VAR=val ... [-- bench args]>" ...
# (bench lines appended to $AB_OUT/<tag>_<k>.jsonl, default ab_out/)
tag=$1; rounds=$2; shift 2
out=${AB_OUT:-ab_out}
mkdir -p $out
for i in $(seq $rounds); do
  k=0
  for setting in "$@"; do
    k=$((k+1))
    envpart="${setting%%--*}"; argpart=""; case "$setting" in *--*) argpart="${setting#*--}";; esac
    env $envpart python bench.py --full --no-cpu-baseline $argpart 2>/dev/null | grep '^{' >> $out/${tag}_$k.jsonl
  done
done
k=0
for setting in "$@"; do k=$((k+1)); python - "$setting" $out/${tag}_$k.jsonl <<'PY'
import json, sys
v = [json.loads(l) for l in open(sys.argv[2])]
print("%-60s" % sys.argv[1], " ".join("%.4f" % d["ms_per_step"] for d in v), "| trace in-frame", " ".join("%.4f" % d["roofline"]["kernel_ms"] for d in v))
PY
done
