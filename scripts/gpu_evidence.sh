#!/bin/bash
# One GPU call of round evidence, in the driver's order: the whole
# `pytest -m gpu` suite once, smoke(), the full bench line, then the
# rocprofv3 passes (scripts/gpu_profile.sh) unless NOPROF=1.
#   bash scripts/gpu_evidence.sh r06a     (results under $EVIDENCE_OUT/r06a, default evidence/)
R=$GRAFT_REPO_ROOT
TAG=${1:-r06}
export EVIDENCE_OUT=${EVIDENCE_OUT:-$R/evidence}
O=$EVIDENCE_OUT/$TAG
cd $R && mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v -p no:cacheprovider --timeout 200 --timeout-method thread \
    > $O/pytest_gpu.log 2>&1 || { tail -60 $O/pytest_gpu.log; exit 1; }
tail -1 $O/pytest_gpu.log
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || exit $?
timeout -k 10 400 python bench.py --full > $O/bench.json 2> $O/bench.err || exit $?
echo bench_ok
[ "${NOPROF:-0}" = 1 ] || bash scripts/gpu_profile.sh $TAG || exit $?
echo evidence_ok
