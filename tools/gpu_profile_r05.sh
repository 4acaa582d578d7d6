#!/bin/bash
# Round-5 profiling recipe of the headline workload (run through gpurun): kernel trace + stats, then PMC passes, each in its
# own run (rocprofv3 --pmc must not be combined with the trace domains on this pool), the FETCH_SIZE calibration, and the
# traffic file bench.py reads (profiles/pmc_traffic_config3.json).
#   tools/gpu_profile_r05.sh <tag> [bench args...]      e.g.  tools/gpu_profile_r05.sh r05_config3
#   CFG=5 CALIB=0 tools/gpu_profile_r05.sh r05_config5 --config 5 --packets 10000000     (another config: the traffic file is named after it)
set -u
CFG=${CFG:-3}; CALIB=${CALIB:-1}
TAG=${1:-r05_config3}; shift || true
ROOT=$(pwd); OUT=$ROOT/gpurun_out/prof_$TAG; mkdir -p "$OUT"; export TMPDIR=/tmp
BENCH="python $ROOT/bench.py --full --steps 1 --warmup 1 --cpu-sample 0 --boundary-packets 0 --no-extra $*"
cd /tmp
timeout -k 5 600 rocprofv3 --kernel-trace --stats -d "$OUT/trace" -o trace -- $BENCH > "$OUT/trace_bench.log" 2>&1
i=0
for c in "FETCH_SIZE" "WRITE_SIZE" \
         "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_ACTIVE_INST_VALU" \
         "TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum TCC_READ_sum" \
         "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_64B_sum" \
         "TA_BUSY_avr TA_TA_BUSY_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum"; do
  i=$((i+1))
  timeout -k 5 600 rocprofv3 --pmc $c -d "$OUT/pmc_$i" -o pmc -- $BENCH > "$OUT/pmc_$i.log" 2>&1
done
[ "$CALIB" = 1 ] && timeout -k 5 300 rocprofv3 --pmc FETCH_SIZE -d "$OUT/calib" -o pmc --output-format csv -- python $ROOT/tools/micro_calib.py > "$OUT/calib.log" 2>&1
cd "$ROOT"
python tools/rocprof_summary.py "$OUT" > "$OUT/summary.txt" 2>&1
python - "$OUT" <<'PY' >> "$OUT/summary.txt" 2>&1
import csv, glob, sys
print("== FETCH_SIZE calibration (tools/micro_calib.py: every lane reads random aligned blocks with 16-byte loads, 1.6 GB table)")
rows = []
for f in glob.glob(sys.argv[1] + "/calib/**/*counter_collection.csv", recursive=True):
    rows += [r for r in csv.DictReader(open(f)) if "microbench" in r.get("Kernel_Name", "") and r["Counter_Name"] == "FETCH_SIZE"]
rows.sort(key=lambda r: int(r["Dispatch_Id"]))
sizes = [16, 16, 32, 32, 64, 64, 128, 128]
for r, s in zip(rows, sizes):
    req = 4096 * 256 * 64 * s
    kib = float(r["Counter_Value"])
    print(f"dispatch {r['Dispatch_Id']}: blocks of {s:3d} B, requested {req / 1e9:7.3f} GB, FETCH_SIZE {kib:.0f} KiB = {kib * 1024 / 1e9:7.3f} GB, ratio FETCH_SIZE/requested {kib * 1024 / req:.3f}")
PY
grep -h '"metric"' "$OUT/trace_bench.log" > "$OUT/bench_line.json"
# traffic of one step of the propagation kernel (all its launches) -> the file bench.py reads
python - "$OUT" "$CFG" <<'PY'
import json, re, sys
out = sys.argv[1]; cfg = sys.argv[2]
per = {}
for line in open(out + "/summary.txt"):
    m = re.match(r"(\S*propagate_wave\S*)\s+(FETCH_SIZE|WRITE_SIZE)\s+dispatches=\s*(\d+)\s+sum_over_dispatches=(\S+)", line)
    if m:
        per.setdefault(m.group(1), {})[m.group(2)] = (float(m.group(4)), int(m.group(3)))
# (a run may hold a second instantiation -- the counting leg of bench.py's v-packet roofline launches the one with the profiling counters:
# the production kernel is the one with the most dispatches)
vals, n = {}, {}
if per:
    prod = max(per, key=lambda k: per[k].get("FETCH_SIZE", (0.0, 0))[1])
    vals = {c: v[0] for c, v in per[prod].items()}; n = {c: v[1] for c, v in per[prod].items()}
line = json.loads(open(out + "/bench_line.json").read().strip().splitlines()[-1])
steps = line["steps"] + line["warmup"]
if len(vals) == 2:
    per_step = (vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0 / steps
    lps = line["roofline"]["launches_per_step"]
    json.dump({"hbm_bytes_per_step": per_step, "hbm_bytes_per_launch": per_step / lps,
               "FETCH_SIZE_KiB_per_step": vals["FETCH_SIZE"] / steps, "WRITE_SIZE_KiB_per_step": vals["WRITE_SIZE"] / steps,
               "launches_profiled": n["FETCH_SIZE"], "kernel": prod, "packets_per_gpu": line["config"]["packets_per_gpu"], "launches_per_step": lps,
               "correction": "none: FETCH_SIZE calibrated on this kernel's access pattern (tools/micro_calib.py under rocprofv3 --pmc FETCH_SIZE, see the "
                             "calibration block of the round's rocprof summary): 64 bytes counted per missed 16/32/64-byte block, i.e. the sectors actually "
                             "fetched; the guide's x2 applies to wide coalesced 128-byte requests, which this kernel does not issue",
               "note": "(FETCH_SIZE + WRITE_SIZE) * 1024 of propagate_wave_kernel, summed over the launches (epochs) of one step; bench.py --config " + cfg + " at packets_per_gpu"},
              open(out + f"/pmc_traffic_config{cfg}.json", "w"), indent=1)
PY
find "$OUT" -name "*.db" -delete
tail -12 "$OUT/summary.txt"
