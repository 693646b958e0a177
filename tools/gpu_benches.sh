# One default-shaped bench line per BASELINE config on one GPU (with the CPU
# baselines and the resolver's stage breakdown), run on the GPU box.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
OUT=${KSG_BENCH_OUT:-$PWD/bench_out}  # (where the lines go)
mkdir -p "$OUT"
for wl in "$@"; do
  timeout -k 10 400 python bench.py --full --workload "$wl" > "$OUT/r2_bench_$wl.json" 2> "$OUT/r2_bench_$wl.err" || exit 1
done
