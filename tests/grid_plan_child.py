"""Child of tests/test_gpu_grid_plans.py: the named cases of tests/grid_plan_cases.py on the GPU in THIS process's environment
(the NDT_K1_* switches are read once per process), one JSON line per case.  A case that fails its checks is reported and the
child goes on; an error ends it.   grid_plan_child.py GROUP [NAME ...]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "16")

import grid_plan_cases as gpc  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from toyslam_amd import ndt  # noqa: E402


def main():
    group, names = sys.argv[1], set(sys.argv[2:])
    for case in gpc.cases_of(group):
        if names and case.name not in names:
            continue
        fails, rep = gpc.check_case(ndt, po, case, placed=False)
        print(json.dumps(dict(name=case.name, fails=fails, build=rep["build"], other_form=rep.get("other_form"),
                              eval_dev=rep.get("eval_dev"), grid_dev=rep.get("grid_dev"))), flush=True)


if __name__ == "__main__":
    main()
