#!/bin/bash
# frames/s of the headline model for batch sizes x row blocks per workgroup (DRNMF_RB); run from the repo root
line=$(mktemp)
for b in 128 256 512 1024; do for rb in 1 2; do
  DRNMF_RB=$rb python bench.py --full --batch $b --frames 200 --no-cpu-baseline --no-ista --no-train --steps 2 --warmup 1 2>/dev/null > "$line"
  python - "$line" <<PY
import json, sys
d=json.load(open(sys.argv[1]))
print(d["config"]["B_per_gpu"], $rb, round(d["value"]), round(d["roofline"]["launch_us"],2), round(d["roofline"]["frac"],3))
PY
done; done
rm -f "$line"
