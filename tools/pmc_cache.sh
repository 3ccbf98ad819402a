# Cache behaviour of the gather kernels (flow_warp*, warp_blend, resize): are the bilinear taps served by L1 / L2 or by HBM?
# Separate rocprofv3 --pmc passes over one forward each; summed per kernel by tools/pmc_lds.py.
cd $GRAFT_REPO_ROOT; export TMPDIR=/tmp
OUT=${OUT:-out}; mkdir -p "$OUT"        # where the outputs go (default: out/ in the repository, git-ignored)
F="--steps 1 --warmup 1 --no-cpu-baseline --no-profile --no-host-io --no-configs"
rm -rf $OUT/cache1 $OUT/cache2 $OUT/cache3 $OUT/cache4
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum -d $OUT/cache1 --output-format csv -- python3 bench.py $F > $OUT/cache1.log 2>&1
rocprofv3 --pmc TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum -d $OUT/cache2 --output-format csv -- python3 bench.py $F > $OUT/cache2.log 2>&1
rocprofv3 --pmc FETCH_SIZE -d $OUT/cache3 --output-format csv -- python3 bench.py $F > $OUT/cache3.log 2>&1
rocprofv3 --pmc GRBM_GUI_ACTIVE -d $OUT/cache4 --output-format csv -- python3 bench.py $F > $OUT/cache4.log 2>&1
python tools/pmc_lds.py $OUT/cache1 $OUT/cache2 $OUT/cache3 $OUT/cache4 > $OUT/cache_summary.txt 2>&1
rm -rf $OUT/cache1 $OUT/cache2 $OUT/cache3 $OUT/cache4
