#!/bin/bash
# The round-5 profiling passes, ALL in one gpurun session (the VALU roofline must be reproducible from one
# session -- the issue-rate microbenchmark, its counters and the tracking kernel's counters are taken on the same box,
# back to back, under one session id that tools/lk_pmc_json.py checks):
#   1  tools/valu_rate: wall time, shader cycles and in-kernel clock per wave-instruction of LK's mix (unprofiled)
#   2  tools/valu_rate --quick under rocprofv3 --pmc: the SAME SQ counters the tracking kernel is priced with
#   3  kernel trace + stats of the bench configuration (4096 keypoints)
#   4  SQ counters, FETCH_SIZE, WRITE_SIZE of the tracking kernel at 4096 and 8192 keypoints (separate --pmc passes)
#   5  the loop-closure side, N frames per set of launches (tools/detector_batch_profile.py), plain and under --stats
#   6  the pose graph alone (4541 vertices, 40 closures)
# rocprofv3 output goes to /tmp; only this library's rows come back under gpurun_out/r05/.
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
export GPU_MAX_HW_QUEUES=8
OUT=gpurun_out/r05
mkdir -p $OUT
SESSION="r05-$(date +%Y%m%dT%H%M%S)-$$"
echo "{\"session\": \"$SESSION\", \"GPU_MAX_HW_QUEUES\": \"$GPU_MAX_HW_QUEUES\", \"lk_hip_sha256\": \"$(sha256sum ros_stereo_slam_amd/csrc/lk.hip | cut -d' ' -f1)\"}" > $OUT/environment.json
keep() { head -1 "$1" > "$2"; grep -v "at::\|elementwise\|vectorized\|Memcpy\|rocprim\|hipcub\|fillBuffer" "$1" | tail -n +2 >> "$2"; }
[ -x tools/valu_rate ] || hipcc --offload-arch=gfx950 -O3 tools/valu_rate.hip -o tools/valu_rate
timeout -k 5 200 tools/valu_rate "$SESSION" > $OUT/valu_rate.jsonl 2> $OUT/valu_rate.err || exit 1
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES --kernel-trace --output-format csv -d /tmp/r05_vr -o vr -- tools/valu_rate "$SESSION" --quick > $OUT/valu_rate_pmc_run.jsonl 2> $OUT/valu_rate_pmc.err || exit 2
cp $(find /tmp/r05_vr -name "vr_counter_collection.csv") $OUT/valu_rate_counter_collection.csv
cp $(find /tmp/r05_vr -name "vr_kernel_trace.csv") $OUT/valu_rate_kernel_trace.csv
[ "$1" = valu ] && exit 0
ARGS="--full --steps 20 --warmup 5 --no-cpu-baseline --no-extras --no-kernel-timing --min-timed-s 0"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/r05_trace -o bench -- python3 bench.py $ARGS > $OUT/trace_bench.json 2> $OUT/trace.err || exit 3
keep $(find /tmp/r05_trace -name "bench_kernel_stats.csv") $OUT/kernel_stats.csv
keep $(find /tmp/r05_trace -name "bench_kernel_trace.csv") $OUT/kernel_trace.csv
for K in ${KPTS:-4096 8192}; do
PARGS="--full --steps 6 --warmup 1 --no-cpu-baseline --no-extras --no-kernel-timing --min-timed-s 0 --kpts $K"
timeout -k 10 400 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VALU --kernel-trace --output-format csv -d /tmp/r05_sq_$K -o sq -- python3 bench.py $PARGS > $OUT/sq_bench_$K.json 2> $OUT/sq_$K.err || exit 4
keep $(find /tmp/r05_sq_$K -name "sq_counter_collection.csv") $OUT/sq_counter_collection_$K.csv
keep $(find /tmp/r05_sq_$K -name "sq_kernel_trace.csv") $OUT/sq_kernel_trace_$K.csv
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d /tmp/r05_fetch_$K -o fetch -- python3 bench.py $PARGS > $OUT/fetch_bench_$K.json 2> $OUT/fetch_$K.err || exit 5
keep $(find /tmp/r05_fetch_$K -name "fetch_counter_collection.csv") $OUT/fetch_counter_collection_$K.csv
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d /tmp/r05_write_$K -o write -- python3 bench.py $PARGS > $OUT/write_bench_$K.json 2> $OUT/write_$K.err || exit 6
keep $(find /tmp/r05_write_$K -name "write_counter_collection.csv") $OUT/write_counter_collection_$K.csv
done
[ "$1" = all ] || { du -sh $OUT; exit 0; }
timeout -k 10 300 python3 tools/detector_batch_profile.py 1400 > $OUT/detector_batch.txt 2> $OUT/detector_batch.err || exit 7
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/r05_det -o det -- python3 tools/detector_batch_profile.py 700 > $OUT/detector_batch_prof.txt 2> $OUT/detector_batch_prof.err || exit 8
grep "cv_\|bow_\|voc_\|lc_\|fr_ransac\|Name" $(find /tmp/r05_det -name "det_kernel_stats.csv") > $OUT/detector_kernel_stats.csv
timeout -k 10 300 python3 tools/pg_profile.py 4541 40 3 > $OUT/pg_plain.log 2>&1 || exit 9
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/r05_pg -o pg -- python3 tools/pg_profile.py 4541 40 1 > $OUT/pg_prof.log 2>&1 || exit 10
grep "pg_\|Name" $(find /tmp/r05_pg -name "pg_kernel_stats.csv") > $OUT/pg_kernel_stats.csv
du -sh $OUT
