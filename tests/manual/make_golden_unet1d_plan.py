"""TEST INFRASTRUCTURE ONLY.  Writes tests/golden/unet1d_plan.json, the recorded launch plan that tests/test_gpu_unet1d_plan.py
compares with (cases, fields and the recording itself live in that module: `CASES`, `record_setting`).  Needs an MI355X.
    python tests/manual/make_golden_unet1d_plan.py [output path]        # well under a minute
The record comes from whichever `cindm_amd` Python finds first and that package's own library (both are printed): to pin the plan
of an EARLIER commit, put that commit's checkout first on PYTHONPATH.  A host-only refactor is checked against the record of the
commit before it; a change that moves the plan on purpose regenerates the record so that the move shows in its diff."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.append(ROOT)                                   # (after PYTHONPATH: see above)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cindm_amd                                        # noqa: E402
from cindm_amd import _ffi, build                       # noqa: E402
import test_gpu_unet1d_plan as P                        # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else P.GOLDEN
    device = torch.device("cuda:0")
    print("package", os.path.dirname(cindm_amd.__file__), "library sources", _ffi.lib().cindm_source_hash().decode()[:12],
          "tree", build.source_hash()[:12], flush=True)
    out = {}
    for config, key, value, rows in P.CASES:
        t0 = time.time()
        out[P.case_id(config, key, value)] = P.record_setting(config, key, value, rows, device)
        print(f"{P.case_id(config, key, value)}: {time.time() - t0:.2f} s", flush=True)
    write_record(out, path)
    print(path, os.path.getsize(path), "bytes")


def write_record(out, path):
    """One line per (case, row count): a plan that moves shows as the few lines it moved in."""
    cases = []
    for cid in sorted(out):
        rows = ",\n".join(f"{json.dumps(r)}: {json.dumps(out[cid][r], sort_keys=True)}" for r in sorted(out[cid], key=int))
        cases.append(f"{json.dumps(cid)}: {{\n{rows}\n}}")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(cases) + "\n}\n")


if __name__ == "__main__":
    main()
