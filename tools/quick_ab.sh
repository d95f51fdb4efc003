#!/bin/bash
# quick A/B of bench.py variants on the GPU box: prints value / ms_per_step / kernel_ms / gpu_ms per variant
set -o pipefail
run() {
  local tag="$1"; shift
  local out; out=$(mktemp -d)
  env "$@" python bench.py --full --no-cpu-baseline > "$out/b.json" 2>"$out/b.err" || { echo "$tag FAILED"; tail -5 "$out/b.err"; rm -rf "$out"; return 1; }
  python - "$tag" "$out/b.json" <<'PY'
import json,sys
j=json.loads(open(sys.argv[2]).read().strip().splitlines()[-1])
w=j['roofline']['whole_evaluation']
print(f"{sys.argv[1]:28s} value {j['value']:.4e} ms/step {j['ms_per_step']:.4f} kernel {j['roofline']['kernel_ms']:.4f} gpu_ms {w['gpu_ms']:.4f} host {w['host_enqueue_ms']:.4f}")
PY
  rm -rf "$out"
}
