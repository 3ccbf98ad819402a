# One gpurun call = one evidence set (same box): bench line, rocprofv3 kernel stats, HBM traffic (two PMC passes).
# (forward counts: bench.py runs 5 set-up forwards -- the third records the launch plan and replays it once for the self-check: 6 forwards
#  of kernels -- then W warm-up and K timed ones: --steps 5 --warmup 2 = 13 forwards, --steps 1 --warmup 1 = 8)
#   bash tools/collect_profiles.sh <tag>        -> $OUT/<tag>_{bench.json,kernel_stats.csv,pmc_hbm_traffic.json}
set -e
TAG=${1:-r04}
cd $GRAFT_REPO_ROOT
OUT=${OUT:-out}; mkdir -p "$OUT"        # where the outputs go (default: out/ in the repository, git-ignored)
export TMPDIR=/tmp
python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench_err.txt
rm -rf $OUT/${TAG}_stats $OUT/${TAG}_fetch $OUT/${TAG}_write
rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_stats --output-format csv -- python3 bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-profile --no-host-io --no-configs > $OUT/${TAG}_stats.log 2>&1
python tools/pmc_summary.py stats $OUT/${TAG}_stats 13 $OUT/${TAG}_kernel_stats.csv > $OUT/${TAG}_stats_summary.txt 2>&1
rocprofv3 --pmc FETCH_SIZE -d $OUT/${TAG}_fetch --output-format csv -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-profile --no-host-io --no-configs > $OUT/${TAG}_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE -d $OUT/${TAG}_write --output-format csv -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-profile --no-host-io --no-configs > $OUT/${TAG}_write.log 2>&1
python tools/pmc_summary.py traffic $OUT/${TAG}_fetch $OUT/${TAG}_write 8 $OUT/${TAG}_pmc_hbm_traffic.json > $OUT/${TAG}_pmc_summary.txt 2>&1
# keep only the summaries (raw traces are large)
rm -rf $OUT/${TAG}_stats $OUT/${TAG}_fetch $OUT/${TAG}_write
