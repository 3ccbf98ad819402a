cd $GRAFT_REPO_ROOT; export TMPDIR=/tmp
OUT=${OUT:-out}; mkdir -p "$OUT"        # where the outputs go (default: out/ in the repository, git-ignored)
F="--steps 1 --warmup 1 --no-cpu-baseline --no-profile --no-host-io --no-configs"
i=0
for set in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY" "SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY" "SQ_VALU_MFMA_BUSY_CYCLES SQ_VALU_MFMA_COEXEC_CYCLES SQ_INSTS_MFMA SQ_INSTS_VALU" "SQ_LDS_CMD_FIFO_FULL SQ_LDS_DATA_FIFO_FULL SQ_INST_LEVEL_LDS SQ_ACTIVE_INST_VMEM" "SQ_VMEM_TA_ADDR_FIFO_FULL SQ_VMEM_TA_CMD_FIFO_FULL SQ_INST_CYCLES_VMEM_RD SQ_ACTIVE_INST_MISC"; do
  i=$((i+1)); rm -rf $OUT/sq$i
  rocprofv3 --pmc $set -d $OUT/sq$i --output-format csv -- python3 bench.py $F > $OUT/sq$i.log 2>&1 || echo "pass $i failed" >> $OUT/sq_summary.txt
done
python tools/pmc_lds.py $OUT/sq1 $OUT/sq2 $OUT/sq3 $OUT/sq4 $OUT/sq5 >> $OUT/sq_summary.txt 2>&1
rm -rf $OUT/sq1 $OUT/sq2 $OUT/sq3 $OUT/sq4 $OUT/sq5
