#!/usr/bin/env python3
"""Records tests/golden/ustep_classes.json: the U step's length classes of the rating set of tests/classes_data.py under every
knob set and precision there, as a solver on the GPU reports them through the public API -- the class names
(Solver.ustep_classes) and, per class, the ratings and users one launch covers (Solver.profile_scope after one update_U) -- and
the CU count of the device they were laid out for.  tests/test_classes.py holds the host-only layout (csrc/pcr_classes.h) to it.

    python tools/record_ustep_classes.py [OUT.json]      (on a machine with the GPU; run at the commit to record)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch

import classes_data as cd
import primalcr_amd as pcr


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ustep_classes.json")
    d1, d2, user, item, val = cd.rating_set()
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    U0, V0 = pcr.initial(d1, cd.K) * 0.2, pcr.initial(d2, cd.K) * 0.2
    rec = {"ncu": torch.cuda.get_device_properties(0).multi_processor_count, "device": torch.cuda.get_device_name(0),
           "ratings": int(len(user)), "users": d1, "cases": {}}
    for prec in cd.PRECISIONS:
        for knobs in cd.KNOB_SETS:
            with pcr.tuned(**knobs):
                s = pcr.Solver(ds, pcr.Parameter(k=cd.K, precision=pcr.PCR_F64 if prec == "f64" else pcr.PCR_F32, **{"lambda": 20.0}))
            s.set_factors(U0, V0)
            s.comp_m(want=False)                                   # (the sorted state update_U starts from)
            s.profile(True)
            s.update_U()
            s.sync()
            classes = []
            for name in s.ustep_classes():
                ratings, users = s.profile_scope(name)
                classes.append({"name": name, "ratings": ratings, "users": users})
            s.close()
            rec["cases"][cd.case_id(prec, knobs)] = classes
            print(cd.case_id(prec, knobs), [c["name"] for c in classes], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
