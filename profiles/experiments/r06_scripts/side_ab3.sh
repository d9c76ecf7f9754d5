#!/bin/bash
cd $GRAFT_REPO_ROOT
for round in 1 2 3; do
  for v in 0 1; do
    echo "IDOCP_SIDE_STREAM=$v"; IDOCP_SIDE_STREAM=$v python bench.py --full --no-cpu-baseline --no-latency --steps 20 2>&1 | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(round(d['ms_per_step'],4), d['config']['step_ms_hip_events']['median'], {k:round(v,3) for k,v in d['config']['kernel_ms'].items()})"
  done
done
python bench.py --full --no-cpu-baseline 2>&1 | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print(round(d['ms_per_step'],4), d['config']['latency'])"
python -m pytest tests -x -q -m gpu 2>&1 | tail -2
