"""The U step's length-class layout (csrc/pcr_classes.h) on the CPU: csrc/check/classes_dump runs the layout function without a
device, and every case must name the classes, in order, with the users and ratings that solvers on an MI355X reported for the
same rating set and knobs (tests/golden/ustep_classes.json, recorded by tools/record_ustep_classes.py through the public API
before the layout moved out of Solver::init)."""
import json
import os
import re

import pytest

import classes_data as cd
from conftest import GOLDEN


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """Builds classes_dump once; dump(precision, knobs, ncu) -> (exit code, parsed classes, scalars, raw output)."""
    exe, tmp = cd.build_dump(), tmp_path_factory.mktemp("classes")
    return lambda precision, knobs, ncu: cd.run_dump(exe, tmp, precision, knobs, ncu)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "ustep_classes.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("knobs", cd.KNOB_SETS, ids=lambda k: cd.case_id("", k).lstrip(",") or "default")
@pytest.mark.parametrize("precision", cd.PRECISIONS)
def test_layout_matches_the_classes_the_gpu_solver_reported(dump, recorded, precision, knobs):
    rc, classes, _, out = dump(precision, knobs, recorded["ncu"])
    assert rc == 0, out
    got = [{"name": c["name"], "ratings": c["nnz"], "users": c["users"]} for c in classes if c["users"] > 0]
    assert got == recorded["cases"][cd.case_id(precision, knobs)]


def test_rating_set_reaches_the_layouts_corners(dump, recorded):
    """What the rating set was designed to produce at 256 CUs: a class left empty, a cluster head, classes in global scratch, the
    2048 class in both forms, a Gram class -- and every user in exactly one class."""
    assert recorded["ncu"] == 256
    assert recorded["users"] == len(cd.lengths()) and recorded["ratings"] == int(cd.lengths().sum())
    rc, classes, scalars, out = dump("f64", {}, 256)
    assert rc == 0, out
    assert any(c["users"] == 0 for c in classes)
    head = [c for c in classes if c["K"] > 1]
    assert len(head) == 1 and head[0] is classes[-1] and head[0]["big"] == 1 and head[0]["name"].endswith("gc")
    assert sum(c["users"] for c in classes) == recorded["users"] and sum(c["nnz"] for c in classes) == recorded["ratings"]
    assert scalars["u_big_blocks"] == head[0]["ugrid"] == head[0]["users"] * head[0]["K"] and scalars["ws"] == 4
    names = {k: [c["name"] for c in v] for k, v in recorded["cases"].items()}
    assert "ustep/512gl" in names["f64,cluster_k=1"] and not any(re.search(r"c$", n) for n in names["f64,cluster_k=1"])
    assert "ustep/512.2048l" in names["f64"] and "ustep/512.2048" in names["f64,ustep_mode=2"]
    assert not any(".2048" in n for n in names["f64,ustep_mode=1"])
    assert names["f32,ustep_gram=64"][0] == "ustep/gram64.64"


@pytest.mark.parametrize("ubins", ["64:128:0", "64:64:0,32:64:0", "1024:256:0", "100:256:1", "x"])
def test_bad_ubins_is_the_solvers_error(dump, ubins):
    rc, _, _, out = dump("f64", {"ubins": ubins}, 256)
    assert rc == 2 and out.strip() == "error -1 bad pcr_tune ubins"        # PCR_ERR_ARG, the text pcr_solver_create reports
