cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${OUT:-$R/build/profile}; mkdir -p $O
rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT -d $O/sq1 --output-format csv -- python $R/bench.py --full --batch 64 --steps 1 --warmup 1 --no-cpu-baseline > $O/sq1.log 2>&1
rocprofv3 --pmc SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAIT_INST_LDS SQ_BUSY_CYCLES SQ_LDS_IDX_ACTIVE -d $O/sq2 --output-format csv -- python $R/bench.py --full --batch 64 --steps 1 --warmup 1 --no-cpu-baseline > $O/sq2.log 2>&1
cd $R && python tools/pmc_summary.py $O/sq1 $O/sq1.txt > /dev/null; python tools/pmc_summary.py $O/sq2 $O/sq2.txt > /dev/null; rm -rf $O/sq1 $O/sq2; tail -2 $O/sq1.log | cut -c1-300
