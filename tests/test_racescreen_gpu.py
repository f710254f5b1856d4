"""Race screens of the counted-wait main loops on the GPU (tests/racescreen.py, DESIGN.md "Race screens"): every case of the table
N_LAUNCH times while a bandwidth-bound kernel runs on a second stream, zero wrong launches allowed - and the positive control: a build
whose wait in front of one structure's LDS reads is one weight tile short (-DPBE_RACE_MUTANT) must be caught in every case of that
structure, in a fresh child process.  Each case writes a line to racescreen_report.txt beside the parity report.

60 clean launches do not exclude a race: the mutants' detection rates in the report are the only calibration of what they do exclude."""
import json
import os
import subprocess
import sys

import pytest
import torch

import racescreen as rs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", [cs.id for cs in rs.cases()])
def test_race_screen(dev, cid):
    cs = rs.case(cid)
    res = rs.run_case(cs, dev)
    rs.report(rs.report_line(res))
    assert res["launches"] == rs.N_LAUNCH
    assert res["wrong"] == 0, rs.report_line(res)


@pytest.mark.parametrize("value", sorted(rs.MUTANTS))
def test_race_mutant_is_caught(dev, value, tmp_path):
    """The screen has power: with the mutant library every case of the structure shows at least one wrong launch of N_LAUNCH, and the
    integer cases' diagnosis names the stale slot.  The child is a fresh process with its own time limit; a child that dies fails the test.

    Cases where the compiler's own vmcnt(0) retires the queue before the counted wait (racescreen.shadowed, read from the shipped ISA:
    the 256x320 gather conv, the 160-column A-stationary tile, A-stationary runs of one tile) run and are reported but cannot show a
    mutant: there it is the shipped program.  Measured on MI355X (profiles/racescreen_report.txt): every other case
    59 - 60 wrong launches of 60, the shadowed ones 0 of 60."""
    lib = rs.mutant_lib(value)
    dst = str(tmp_path / "mutant.json")
    env = dict(os.environ, PBE_LIB_PATH=lib, PYTHONPATH=os.pathsep.join([rs.ROOT, os.path.dirname(os.path.abspath(__file__))]))
    try:
        r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "racescreen.py"), str(value), dst],
                           env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:                            # counts as a hang: nothing more is started on this GPU
        pytest.exit(f"mutant {value}: the child ran into its time limit", returncode=1)
    if r.returncode < 0 or r.returncode in (134, 139):           # the child died on a signal: nothing more is started on this GPU
        pytest.exit(f"mutant {value}: the child ended with {r.returncode}\n{r.stderr[-4000:]}", returncode=1)
    assert r.returncode == 0, f"mutant {value}: the child ended with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    with open(dst) as f:
        results = json.load(f)
    assert [x["case"] for x in results] == [cs.id for cs in rs.mutant_cases(value)]
    for x in results:
        rs.report(f"mutant {value} | {x['case']}: {x['wrong']} of {x['launches']} launches wrong ({x['wrong'] / x['launches']:.2f}), {x['seconds']:.2f} s | {x['diagnosis'] or ('shadowed: ' + x['shadowed'] if x['shadowed'] else '')}")
    missed = [x["case"] for x in results if x["wrong"] == 0 and not x["shadowed"]]      # (racescreen.shadowed: the mutant is the shipped program there)
    assert not missed, f"mutant {value} was not caught in {missed}: the screen is too weak there"
    unnamed = [x["case"] for x in results if x["wrong"] and rs.case(x["case"]).family == "int" and rs.case(x["case"]).kind != "ex" and not x["stale"]]
    assert not unnamed, f"mutant {value}: the diagnosis names no stale slot in {unnamed}"
