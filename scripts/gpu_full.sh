#!/bin/bash
# On the GPU box: the -m gpu suite (no -x: every failure reported), smoke(), the full bench line (--full: with
# the dominant kernel's roofline and the CPU baseline) and a rocprofv3 kernel-trace of a short plain bench run.
# TAG names the logs; they go to $OUT_DIR (default: build/logs under the repository).
set -o pipefail
R=${GRAFT_REPO_ROOT:-/root/repo}
TAG=${1:-x}
O=${OUT_DIR:-$R/build/logs}
cd $R && mkdir -p $O
timeout -k 10 700 python -u -m pytest tests -m gpu -q -rf --timeout 300 --timeout-method thread > $O/tests_$TAG.log 2>&1
rc=$?
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc   # 1 = test failures (reported); anything else ends the call
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$TAG.log 2>&1 && \
timeout -k 10 300 python bench.py --full > $O/bench_$TAG.json 2> $O/bench_$TAG.err && \
cd /tmp && export TMPDIR=/tmp && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_$TAG -o prof --output-format csv -- python3 $R/bench.py --steps 5 --warmup 2 > $O/prof_$TAG.log 2>&1 && \
exit $rc
