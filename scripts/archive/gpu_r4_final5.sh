#!/bin/bash
# Round-4 final state: smoke, GPU suite, the BASELINE-size RCCL rank-process runs (GP_MPROC_FULL=1),
# bench (traffic + CPU baseline), kernel trace.
export TMPDIR=/tmp
O=${O:-gpurun_out/r4_final5}
mkdir -p $O
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1 || { tail -20 $O/smoke.log; exit 1; }
tail -1 $O/smoke.log
timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 600 --timeout-method thread --durations=30 > $O/pytest_gpu.log 2>&1
rc=$?; grep -E "passed|failed" $O/pytest_gpu.log | tail -2; grep FAILED $O/pytest_gpu.log | head; [ $rc = 0 ] || exit $rc
GP_MPROC_FULL=1 timeout -k 10 600 python -u -m pytest tests/test_gpu_rccl_multiproc.py -v -k baseline_size --timeout 500 --timeout-method thread > $O/mproc_full.log 2>&1 || { tail -30 $O/mproc_full.log; exit 1; }
grep -E "passed|failed" $O/mproc_full.log | tail -1
timeout -k 10 600 python -u bench.py --full > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 1; }
cat $O/bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_kt -o kt -- python3 bench.py --no-cpu --no-traffic --steps 20 --warmup 2 > $O/bench_kt.json 2> $O/bench_kt.err || { tail -20 $O/bench_kt.err; exit 1; }
python3 tools/kt_steady.py $O/prof_kt k_ps_tile --last 20
