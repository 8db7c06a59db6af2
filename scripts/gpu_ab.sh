#!/bin/bash
# quick A/B pass on the GPU box: the GEMM / epilogue parity tests, then the
# C2 bench line under each variant given as "NAME=VALUE ..." arguments
R=$GRAFT_REPO_ROOT
O=${EVIDENCE_OUT:-$R/evidence}
cd $R && mkdir -p $O
timeout -k 10 300 python -u -m pytest tests/test_gpu_kernels.py tests/test_gpu_protocols.py -m gpu -x -q -p no:cacheprovider --timeout 150 --timeout-method thread -k "mul or gemm or trunc or session" > $O/pytest_ab.log 2>&1 || exit $?
echo tests_ok
i=0
for v in "$@"; do
  i=$((i+1))
  env $v timeout -k 10 120 python bench.py --full --no-extras --no-binary --no-cpu-baseline --steps 100 > $O/ab_$i.json 2> $O/ab_$i.err || exit $?
  echo "$v $(python3 -c "import json;d=json.load(open('$O/ab_$i.json'));print(round(d['ms_per_step'],4), d['kernel_ms_per_step'], round(d['roofline']['frac'],3))")"
done
