#!/bin/bash
# the full bench line (--full) three times -> OUT/<tag>_bench_full_{1,2,3}.json (+ OUT/profiles_<tag>/ copies)
#   bash tools/bench_full3.sh r06 OUT
TAG="${1:-r05}"
OUT="${2:?usage: bash tools/bench_full3.sh TAG OUT_DIR}"
cd "$(dirname "${BASH_SOURCE[0]}")/.."
mkdir -p "$OUT/profiles_${TAG}"
for i in 1 2 3; do
  python bench.py --gpus 1 --steps 20 --warmup 5 --full > "$OUT/${TAG}_bench_full_$i.json" 2> "$OUT/${TAG}_bench_full_$i.err"
  echo "run $i rc $?"
  cp "$OUT/${TAG}_bench_full_$i.json" "$OUT/profiles_${TAG}/${TAG}_bench_full_run$i.json"
done
cp "$OUT/${TAG}_bench_full_1.json" "$OUT/profiles_${TAG}/${TAG}_bench_full.json"
python - "$OUT" "$TAG" <<'PY'
import json, sys
out, tag = sys.argv[1], sys.argv[2]
for i in (1, 2, 3):
    j = json.loads([l for l in open("%s/%s_bench_full_%d.json" % (out, tag, i)) if l.startswith("{")][-1])
    r = j["roofline"]
    print(i, j["value"], r["kernel_ms"], r["frac"], r.get("profile_mismatch"), {k: v.get("roofline", {}).get("kernel_ms") for k, v in j["secondary"].items() if isinstance(v, dict)})
PY
