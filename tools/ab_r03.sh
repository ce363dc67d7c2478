#!/bin/bash
# same-box A/B of trees built in the container under _ab/ against the working tree:  tools/ab_r03.sh <tag> <rounds> <tree>...   ("." = the working tree)
# (bench lines appended to $AB_OUT/<tag>_<tree>.jsonl, default ab_out/)
tag=$1; rounds=$2; shift 2
out=${AB_OUT:-ab_out}
mkdir -p $out
for i in $(seq $rounds); do
  for t in "$@"; do
    name=$(echo $t | tr '/. ' '___')
    if [ "$t" = "." ]; then python bench.py --full --no-cpu-baseline 2>/dev/null | grep "^{" >> $out/${tag}_new.jsonl
    elif [ "$t" = ".fused" ]; then python bench.py --full --no-cpu-baseline --tone-map fused 2>/dev/null | grep "^{" >> $out/${tag}_new_fused.jsonl
    else full=$(grep -q -- '"--full"' _ab/$t/bench.py && echo --full)      # (trees older than the option print the full line by default)
      (cd _ab/$t && python bench.py $full --no-cpu-baseline 2>/dev/null | grep '^{') >> $out/${tag}_$name.jsonl; fi
  done
done
python - $tag $out <<'PY'
import json, glob, os, sys
for f in sorted(glob.glob(os.path.join(sys.argv[2], "%s_*.jsonl" % sys.argv[1]))):
    v = [json.loads(l) for l in open(f)]
    print("%-40s" % f.split("/")[-1], " ".join("%.4f" % d["ms_per_step"] for d in v), "| trace in-frame", " ".join("%.4f" % d["roofline"]["kernel_ms"] for d in v), "| waves", " ".join(str(d["config"].get("trace_workgroup_waves")) for d in v))
PY
