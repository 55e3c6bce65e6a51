"""What plan_resolve (csrc/rae_plan.hpp) decides, without a GPU: tests/plan_dump.hip prints every
scalar of the kernel arguments, every form / geometry field, the workspace size and each
workspace pointer's offset for one config; tests/golden/plan_specs.json holds the same lines as
the commit before the resolve / allocate split computed them inside rae_plan_create (the
configs and the recorded lines, nothing else).  plan_dump also binds a copy of the spec to a
real range and exits non-zero unless every pointer lands on base + its offset."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
with open(os.path.join(GOLDEN, "plan_specs.json")) as _fh:
    SPECS = json.load(_fh)


@pytest.fixture(scope="session")
def plan_dump(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "plan_dump"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-host-only",
                    os.path.join(ROOT, "tests", "plan_dump.hip"), "-o", str(exe)], check=True)
    return str(exe)


def test_matrix_covers_every_rejection_and_form():
    """The fixture holds one config per rejection message of plan_resolve and both outcomes of
    every form the plan resolves.  ("update grid too large" has none: with the exchange buffer
    below 2^30 floats (4 GiB: the records' 32-bit byte offsets) and at most RAE_IDX_HMAX *
    RAE_IDX_PART records per table, update_grid stays below 2048 + 1 + 2^20 / 17 + 6144 +
    4 * 2^30 / 12 < 2^31.)"""
    src = open(os.path.join(ROOT, "relation-autoencoder_amd", "csrc", "rae_plan.hpp")).read()
    body = src[src.index("inline int plan_resolve("):]
    n_fail = body.count("return fail(")
    errs = {e["lines"][1] for e in SPECS if e["lines"][0] != "rc 0"}
    assert len(errs) == n_fail - 1, (n_fail, sorted(errs))
    ok = [dict(l.split(" ", 1) for l in e["lines"]) for e in SPECS if e["lines"][0] == "rc 0"]
    for key in ("v4", "sp_split", "mt_bf16", "mt_direct", "bf16", "fuse_prep", "priv", "privc",
                "part", "pipe", "reg_on", "dpart", "vb_is_ex", "dwb_is_ex"):
        assert {d[key] for d in ok} == {"0", "1"}, key
    assert {d["q"] for d in ok} == {"1", "2"}
    assert {d["dp2"] for d in ok} == {"0", "1", "2"}
    assert {d["lay.wire"] for d in ok} == {"0", "1", "2"}
    assert {d["hch"] for d in ok} == {"0", "128"}
    assert {d["off.args.mtP"] == "-1" for d in ok} == {True, False}


@pytest.mark.parametrize("spec", SPECS, ids=[e["name"] for e in SPECS])
def test_plan_resolve_matches_recorded_plan(plan_dump, spec):
    args = [f"{k}={v}" for k, v in spec["config"].items()]
    p = subprocess.run([plan_dump, *args], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = p.stdout.splitlines()
    for g, w in zip(got, spec["lines"]):
        assert g == w
    assert len(got) == len(spec["lines"])
