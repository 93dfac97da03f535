#!/bin/bash
# A/B of the `replicas` leg (K matches per call) under the two device-chain forms, on the GPU box -> $OUT (default bench_out/r05)
out=${OUT:-bench_out/r05}
mkdir -p $out
for cm in 1 2; do
  timeout 400 python bench.py --full --legs replicas --no-cpu --chain-mode $cm --steps 64 > $out/rep_cm$cm.json 2> $out/rep_cm$cm.err
  python - <<PY
import json
try:
    d = json.loads(open("$out/rep_cm$cm.json").read().strip().splitlines()[-1])
    print("chain mode $cm: headline %.4f ms/step" % d["ms_per_step"])
    for r in d["replicas"]["by_K"]:
        print("  K %2d: %.3f ms/call, %.2f G units/s, frac %.3f, %.1f us/launch, kernels/call %s, spec %.2f, resident %s/%s" % (
            r["K"], r["ms_per_call"], r["value"] / 1e9, r["roofline"]["frac"], r["roofline"]["avg_launch_us"],
            r["kernels_per_call"], r["speculation_ratio"], r.get("co_resident_launches"), r.get("co_resident_gave_up")))
except Exception as e:
    print("chain mode $cm: no line (%s)" % e)
PY
  tail -2 $out/rep_cm$cm.err
done
