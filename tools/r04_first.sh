#!/bin/bash
# round 4, first GPU call: counter list, GPU tests, baseline bench line
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
O=${OUT:-bench_outputs}/r04; mkdir -p $O
rocprofv3 -L > $O/counters.txt 2>&1
python3 -m pytest tests -m gpu -x -q > $O/pytest.log 2>&1; echo "pytest rc $?" &&
tail -3 $O/pytest.log &&
python3 bench.py --full > $O/bench_base.json 2> $O/bench_base.err && cut -c1-600 $O/bench_base.json
