#!/bin/bash
# usage (GPU box): tools/ab_bench.sh ab/<variant> [ab/<variant> ...]
# A/B of kernel variants ON ONE BOX: boxes differ by +-3 % in bench.py's value, more than most single changes are worth.
# Build each variant in the container (python -m popsift_amd.build), copy popsift_amd/lib/libpopsift_hip.so to
# ab/<variant>/ (ab/ travels with the snapshot; do not commit it), then run this with the variants listed twice in
# alternating order.  Prints value / sparse / caller / device-resident / single-frame per run.
cd $GRAFT_REPO_ROOT
set -o pipefail
W=$(mktemp -d) || exit 1
cp popsift_amd/lib/libpopsift_hip.so "$W/libpopsift_hip.keep" || exit 1
for v in "$@"; do
    cp $v/libpopsift_hip.so popsift_amd/lib/libpopsift_hip.so || break
    # one run per variant under a time limit; a failed run ends the A/B (the library is put back below)
    timeout -k 10 600 python bench.py --full --no-cpu-baseline --no-parity 2>"$W/ab.err" | tail -1 > "$W/ab_line.json" \
      || { echo "$v: bench.py failed (exit $?)"; tail -5 "$W/ab.err"; break; }
    python - "$v" "$W/ab_line.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
print(sys.argv[1], d["value"], {k: (v.get("value") if isinstance(v, dict) else v) for k, v in d.items()
      if k in ("sparse_frames", "caller_profile", "device_resident", "single_frame")}, "k_blur frac", d["roofline"]["frac"],
      "stages", d["stage_ms_single_frame"])
PY
done
cp "$W/libpopsift_hip.keep" popsift_amd/lib/libpopsift_hip.so
