#!/bin/bash
# A/B of library BUILDS on the benchmark frame: every build (a path to a libgvt_hip*.so, optionally "path:opt=v,opt=v") is run `reps` times, alternating, through
# bench.py's per-kernel HIP events.   bash tools/ab_lib.sh reps lib1[:opts] lib2[:opts] ...
# Every bench.py run has a time limit of its own (AB_TIMEOUT seconds, default below).  The script STOPS at the first run that fails -- a non-zero exit status, the
# time limit, or no result line -- with a non-zero exit status of its own: nothing more is started on a device a run may have left in a bad state.
reps=$1; shift
limit=${AB_TIMEOUT:-60} # a plain run of the command line below takes about 3 s on an idle MI355X: twenty times that for a loaded, shared machine
log=${OUT_DIR:-out}/ab/ab.log # (OUT_DIR: where the measurement scripts under tools/ write)
mkdir -p "$(dirname "$log")"
for r in $(seq 1 "$reps"); do
  for spec in "$@"; do
    lib=${spec%%:*}; opts=""; [ "$lib" != "$spec" ] && opts=${spec#*:}
    args="--full"; for kv in ${opts//,/ }; do args="$args --opt $kv"; done
    GVT_HIP_LIB=$PWD/$lib timeout -k 10 "$limit" python bench.py --steps 40 --warmup 5 --no-cpu-baseline --no-abi-path --no-sustained $args > "$log" 2>&1
    rc=$?
    if [ $rc -ne 0 ]; then
      printf '%-60s FAILED: bench.py ended with status %d (124 / 137: the %s s limit)\n%s\n' "$spec" $rc "$limit" "$(tail -c 400 "$log")"
      exit 1
    fi
    python - "$spec" "$log" <<'PY' || exit 1
import json, sys
l=[x for x in open(sys.argv[2]) if x.startswith("{")]
if not l:
    print("%-60s FAILED: no result line: %s" % (sys.argv[1], open(sys.argv[2]).read()[-400:])); sys.exit(1)
j=json.loads(l[-1]); k=j["roofline"]["kernel_ms"]; s=j["steps"]
print("%-60s frame %.4f ms  closest %.4f long %.4f any %.4f  value %.0f" % (sys.argv[1], j["ms_per_step"], k["ms_closest"]/s, k["ms_long"]/s, k["ms_any"]/s, j["value"]))
PY
  done
done
