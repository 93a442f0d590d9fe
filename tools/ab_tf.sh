#!/bin/bash
# tools/ab_tf.sh <tag> <lib.so> ...: temporal-filter stage time and result checksum of the headline bench for several library builds
while [ $# -ge 2 ]; do
    tag=$1; lib=$2; shift 2
    SVTAV1_HIP_LIB=$lib python bench.py --full --steps 3 --warmup 1 --no-pmc --no-cpu-baseline > /tmp/abtf_$tag.json 2> /tmp/abtf_$tag.err
    python - "$tag" <<'PY'
import json, sys
d = json.load(open(f"/tmp/abtf_{sys.argv[1]}.json"))
for r in d["roofline_all"]:
    if "tf_" in r["kernel"] or "tpl" in r["kernel"]:
        print(sys.argv[1], r["kernel"][:40], r["launch_ms"], r.get("result_checksum"))
PY
done
