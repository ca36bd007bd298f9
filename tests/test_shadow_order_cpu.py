"""No GPU: the child order of the any-hit shadow rays, priced by the walk model (scripts/dev/bvh4_walk_model.cpp - a scalar walk of the tree kz_build_bvh and
kz_collapse_bvh4 make, under the rules of kz_wf_trace). Built here with the host compiler and run on a 20 000-triangle soup with seed 1: descending into the
child that holds most of the segment visits fewer packets per any-hit ray than descending into the nearest entry, and both orders give every ray the same
answer - which occluder is found first does not matter to "occluded"."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nano-kazen_amd", "csrc")
RAYS = 20000


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk_model") / "bvh4_walk_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "scripts", "dev", "bvh4_walk_model.cpp"),
                           os.path.join(CSRC, "kz_bvh.cpp"), "-pthread", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def walks(model, tmp_path_factory):
    """{rule: (the model's record, one '0' / '1' per any-hit ray)} on the 20 000-triangle soup, seed 1."""
    out = {}
    d = tmp_path_factory.mktemp("walks")
    for rule in ("nearest", "overlap"):
        occ = str(d / (rule + ".occ"))
        rec = json.loads(subprocess.check_output([model, "20000", rule, "1", str(RAYS), "-2", occ], text=True))
        out[rule] = (rec, open(occ, "rb").read())
    return out


def test_largest_overlap_visits_fewer_packets_than_nearest_entry(walks):
    near, over = walks["nearest"][0], walks["overlap"][0]
    print("any-hit rays, packets / triangle tests per ray: nearest entry %.2f / %.2f, largest overlap %.2f / %.2f" %
          (near["anyhit"]["packets"], near["anyhit"]["tests"], over["anyhit"]["packets"], over["anyhit"]["tests"]))
    assert near["triangles"] == over["triangles"] == 20000 and near["rays"] == over["rays"] == RAYS and near["packets4"] == over["packets4"] > 0
    assert over["anyhit"]["packets"] < near["anyhit"]["packets"]
    # the rule is the any-hit rays' alone: the closest-hit rays walk as they did
    assert over["closest"] == near["closest"] and near["closest"]["packets"] > 0


def test_both_orders_answer_every_ray_alike(walks):
    near, over = walks["nearest"][1], walks["overlap"][1]
    assert len(near) == len(over) == RAYS and set(near) <= {ord("0"), ord("1")}
    assert near == over
    assert 0 < near.count(b"1") < RAYS          # occluded and free rays both occur


def test_the_model_refuses_what_it_does_not_know(model):
    assert subprocess.run([model, "100", "sideways"], capture_output=True).returncode == 2
    assert subprocess.run([model], capture_output=True).returncode == 2
