cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
O=${OUT_DIR:-prof_out}/r01b   # where the outputs go (OUT_DIR, default prof_out/ in the tree)
mkdir -p $O
timeout 300 python bench.py --full > $O/bench.json 2> $O/bench.err
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/kstats -o k -- python3 bench.py --full --steps 300 --warmup 150 --no-cpu-baseline --no-fp32 > $O/kstats.log 2>&1
timeout 240 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/fetch -o f -- python3 bench.py --full --steps 4 --warmup 1 --no-cpu-baseline --no-fp32 > $O/fetch.log 2>&1
timeout 240 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/write -o w -- python3 bench.py --full --steps 4 --warmup 1 --no-cpu-baseline --no-fp32 > $O/write.log 2>&1
./tools/ubench_overlap > $O/ubench_overlap.txt 2>&1
ls -R $O | head -30
# the float path's kernel: HBM traffic of one 2^24-sample block (same two PMC passes)
timeout 240 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/f32fetch -o f -- python3 tools/bench_f32.py --iters 3 > $O/f32fetch.log 2>&1
timeout 240 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/f32write -o w -- python3 tools/bench_f32.py --iters 3 > $O/f32write.log 2>&1
