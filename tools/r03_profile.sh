# Round-3 profile collection (GPU box): bash tools/r03_profile.sh OUT -> OUT/, folded by python3 tools/r03_collect_profiles.py OUT
set -e
out=$(realpath -m "${1:?usage: bash tools/r03_profile.sh OUTPUT_DIR}")
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
mkdir -p $out
# 1. kernel-trace + stats of the headline command (no secondary / fp32 reference: per-kernel averages are the headline's)
rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats -- python3 bench.py --steps 20 --warmup 3 --full --no-secondary --no-fp32-reference --sustained-seconds 0 > $out/bench_headline.json 2> $out/stats.err
echo stats done
# 2. the same with the secondary configurations (split decoders, table decode, bits path)
rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats_all -- python3 bench.py --steps 20 --warmup 3 --full --no-cpu-baseline --sustained-seconds 0 > $out/bench_all.json 2> $out/stats_all.err
echo stats_all done
# 3. HBM-side traffic, one counter per pass
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --kernel-trace --output-format csv -d $out/pmc_default_$c -- python3 bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-fp32-reference --no-secondary --sustained-seconds 0 > /dev/null 2> $out/pmc_default_$c.err
  rocprofv3 --pmc $c --kernel-trace --output-format csv -d $out/pmc_split_$c -- python3 tools/bench_split_dec.py > /dev/null 2> $out/pmc_split_$c.err
  echo $c done
done
find $out -name "*.csv" | head -40
du -sh $out
