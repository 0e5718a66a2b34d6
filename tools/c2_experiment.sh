#!/bin/bash
# the configs[2] / configs[3] legs of bench.py, a few runs on one box: tools/c2_experiment.sh [runs]
set -u
OUT=${OUT:-out}/c2
mkdir -p $OUT
for r in $(seq 1 ${1:-2}); do
  timeout -k 10 300 python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-kpts8192 --no-host-images > $OUT/b_$r.json 2> $OUT/b_$r.err || { echo fail; tail -5 $OUT/b_$r.err; exit 1; }
  python3 -c "
import json
d=json.loads(open('$OUT/b_$r.json').read().strip().splitlines()[-1])
c=d['configs2']; e=d['end_to_end']
print('value', round(d['value']), 'configs2', round(c['configs2_frames_per_s']), 'side by side', round(c['front_end_and_detector_side_by_side_s'],4), 'fe done', round(c['front_end_done_s'],4), 'det done', round(c['detector_done_s'],4), 'det submitted', round(c['detector_submitted_s'],4), 'first 64 verdicts', round(c['detector_first_64_verdicts_s'],4), flush=True)
print('  end_to_end_s', round(e['end_to_end_s'],4), round(e['end_to_end_frames_per_s']), {k: round(v,4) for k,v in e['rank0_stage_s'].items()}, flush=True)"
done
