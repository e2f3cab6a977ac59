#!/bin/bash
# The labelled f16 throughput mode: bench line, rocprofv3 kernel trace of the same command, PMC passes of the point-block kernel
# (separate passes per counter group, kernel trace only) -> OUT_DIR (copied to profiles/r05_bench_f16*.{json,md}, r05_dvis_f16p_pmc.md)
# usage: bash tools/run_f16_profiles.sh OUT_DIR
O=$(realpath -m "${1:?usage: bash tools/run_f16_profiles.sh OUT_DIR}")
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
mkdir -p $O
timeout 900 python bench.py --full --precision f16 --steps 3 --warmup 1 --no-cpu-baseline > $O/bench_f16.json 2> $O/bench_f16.err
tail -1 $O/bench_f16.json | cut -c1-1500
rocprofv3 --kernel-trace --stats -d $O/prof -o trace -- python bench.py --precision f16 --steps 2 --warmup 1 --no-cpu-baseline --no-legs --no-configs > $O/prof.log 2>&1
python tools/rocpd_summary.py $(find $O/prof -name '*.db' | head -1) > $O/kernel_stats.md
rm -rf $O/prof
head -14 $O/kernel_stats.md
P=f16x1; N=64
run() {
  local name=$1; shift
  rocprofv3 --pmc "$@" --kernel-trace -d $O/$name -o p -- python tools/prof_dvis.py $P $N > $O/$name.log 2>&1
  python tools/rocpd_summary.py $(find $O/$name -name "*.db" | head -1) | grep -i "dvis_f16p\|dvis_pb" >> $O/pmc.md
  rm -rf $O/$name
}
: > $O/pmc.md
run a SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAIT_INST_LDS
run b SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VALU SQ_INSTS_VMEM_RD SQ_INSTS_SALU
run c FETCH_SIZE
run d WRITE_SIZE
run g GRBM_GUI_ACTIVE
cat $O/pmc.md
