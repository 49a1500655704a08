#!/bin/bash
# SQ / LDS counters of the channel kernel, two passes (no other trace domains together with --pmc)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${OUT_DIR:-prof_out}/pmc   # where the outputs go (OUT_DIR, default prof_out/ in the tree)
mkdir -p $O
timeout 240 rocprofv3 --pmc SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAVE_CYCLES --kernel-trace --output-format csv -d $O/p1 -o p -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-fp32 > $O/p1.log 2>&1
timeout 240 rocprofv3 --pmc SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS --kernel-trace --output-format csv -d $O/p2 -o p -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-fp32 > $O/p2.log 2>&1
timeout 240 rocprofv3 --pmc SQ_INSTS_VALU_MFMA_I8 SQ_INSTS_MFMA SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_FLAT SQ_INST_CYCLES_VMEM SQ_WAIT_INST_ANY SQ_THREAD_CYCLES_VALU --kernel-trace --output-format csv -d $O/p3 -o p -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-fp32 > $O/p3.log 2>&1
ls $O/*
