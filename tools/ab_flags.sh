#!/bin/bash
# A/B of bench.py FLAG SETS on ONE GPU box: tools/ab_flags.sh ROUNDS "flags a" "flags b" ...
set -u
cd "$GRAFT_REPO_ROOT" || exit 1
ROUNDS=$1; shift
OUT=${OUT:-out}/abflags
mkdir -p $OUT
for r in $(seq 1 "$ROUNDS"); do
  i=0
  for f in "$@"; do
    i=$((i+1))
    timeout -k 10 400 python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-extras --no-kernel-timing $f > $OUT/${i}_$r.json 2> $OUT/${i}_$r.err || { echo "[$f] round $r failed"; tail -5 $OUT/${i}_$r.err; exit 1; }
    python3 -c "
import json
d=json.loads(open('$OUT/${i}_$r.json').read().strip().splitlines()[-1])
print('[$f]', $r, round(d['value']), flush=True)" || exit 1
  done
done
