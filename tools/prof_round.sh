cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
# usage (from the repo root): tools/prof_round.sh <outdir> [--no-pmc]
out=${1:?usage: tools/prof_round.sh <outdir> [--no-pmc]}; shift
mkdir -p "$out"
rocprofv3 --kernel-trace --stats -d "$out/trace" -- python3 bench.py --steps 5 --warmup 2 --full --no-cpu-baseline > "$out/bench.json" 2> "$out/bench.err"
python3 tools/rocpd_kernel_stats.py "$(find "$out/trace" -name '*.db' | head -1)" > "$out/kernel_stats.txt" 2>&1
head -30 "$out/kernel_stats.txt"
if [ "$1" != "--no-pmc" ]; then
tools/prof_pmc.sh "$out/pmc" > /dev/null 2>&1
python3 tools/pmc_summary.py "$out/pmc" agg_hash dense_probe dense_build > "$out/pmc_summary.txt" 2>&1
head -80 "$out/pmc_summary.txt"
fi
rm -rf "$out/trace"
