# A/B of two builds of the library in one call: bash profiles/probes/ab_lib.sh <other lib> <workload> <arith> [steps] [alternations]
# Runs alternate this tree's library and the other one (default twice each); every bench.py run has its own time limit, and a run
# that fails or exceeds it ends the call.  (--full: kernel_ms_per_step comes from bench.py's profiled pass.)
cd "$(dirname "$0")/../.." || exit 1
for ((a = 0; a < ${5:-2}; a++)); do
  for v in "TTX_DUMMY=1" "TTX_LIB=$PWD/$1"; do
    out=$(env $v timeout -k 10 300 python3 bench.py --workload $2 --arith $3 --steps ${4:-3} --warmup 1 --full --no-cpu-baseline --no-extras 2>/dev/null) || { echo "== ${v:0:9} $2 $3: bench.py ended with status $?"; exit 1; }
    echo "== ${v:0:9} $2 $3: $(echo "$out" | python3 -c 'import json,sys; j=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(round(j["ms_per_step"],3), "ms", j["config"]["integral"], {k: round(v,2) for k,v in j["kernel_ms_per_step"].items()})')"
  done
done
