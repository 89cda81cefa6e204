#!/bin/bash
# usage (GPU box): tools/env_ab.sh 'NAME=VALUE ...' 'NAME=VALUE ...'   -- bench.py's timed legs under each runtime environment ('' = default)
cd $GRAFT_REPO_ROOT
set -o pipefail
W=$(mktemp -d) || exit 1
for v in "$@"; do
  # one run per environment under a time limit; a failed run ends the A/B
  timeout -k 10 600 env $v python bench.py --full --no-extras --steps 10 --warmup 2 2>"$W/env_ab.err" | tail -1 > "$W/env_ab_line.json" \
    || { echo "$v: bench.py failed (exit $?)"; tail -5 "$W/env_ab.err"; exit 1; }
  python - "$v" "$W/env_ab_line.json" <<'PY'
import json, sys
try:
    d = json.load(open(sys.argv[2]))
    print("%-60s value %8.1f  device_resident %8.1f  host_export %8.1f  pcie %s" % (sys.argv[1] or "(default)", d["value"], d["device_resident"]["value"], d["host_export"]["value"], d.get("pcie_gbs", {}).get("d2h")))
except Exception as e:
    print(sys.argv[1], "failed", e)
PY
done
