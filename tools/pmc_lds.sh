cd $GRAFT_REPO_ROOT; export TMPDIR=/tmp
OUT=${OUT:-out}; mkdir -p "$OUT"        # where the outputs go (default: out/ in the repository, git-ignored)
rm -rf $OUT/lds1 $OUT/lds2 $OUT/lds3
F="--steps 1 --warmup 1 --no-cpu-baseline --no-profile --no-host-io --no-configs"
rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d $OUT/lds1 --output-format csv -- python3 bench.py $F > $OUT/lds1.log 2>&1
rocprofv3 --pmc SQ_LDS_ADDR_CONFLICT SQ_LDS_UNALIGNED_STALL -d $OUT/lds2 --output-format csv -- python3 bench.py $F > $OUT/lds2.log 2>&1
rocprofv3 --pmc SQ_INSTS_LDS SQ_ACTIVE_INST_LDS -d $OUT/lds3 --output-format csv -- python3 bench.py $F > $OUT/lds3.log 2>&1
python tools/pmc_lds.py $OUT/lds1 $OUT/lds2 $OUT/lds3 > $OUT/lds_summary.txt 2>&1
rm -rf $OUT/lds1 $OUT/lds2 $OUT/lds3
