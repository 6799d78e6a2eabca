# Round-2 profile collection (GPU box): bash tools/r02_profile.sh OUT -> OUT/, folded by python3 tools/r02_collect_profiles.py OUT
set -e
out=$(realpath -m "${1:?usage: bash tools/r02_profile.sh OUTPUT_DIR}")
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
mkdir -p $out
# kernel-trace + stats of the headline command (no secondary / fp32 reference: per-kernel averages are the headline's)
rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats -- python3 bench.py --steps 20 --warmup 3 --full --no-secondary --no-fp32-reference > $out/bench_headline.json 2> $out/stats.err
echo stats done
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --kernel-trace --output-format csv -d $out/pmc_default_$c -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-fp32-reference --no-secondary > /dev/null 2> $out/pmc_default_$c.err
  rocprofv3 --pmc $c --kernel-trace --output-format csv -d $out/pmc_fused_$c -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-fp32-reference --no-secondary --latent-path fused > /dev/null 2> $out/pmc_fused_$c.err
  echo $c done
done
find $out -name "*.csv" | head -30
du -sh $out
