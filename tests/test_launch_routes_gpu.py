"""What every launch route chooses, against a recorded manifest (-m gpu).

tests/golden/launch_routes.json is the output of tools/dump_routes.py on the MI355X, taken before launch selection in
csrc/fastsvc_plan.cpp was restructured: per case the (layer, kernel, tiles per workgroup) of every launch of a profiled
forward, in launch order - the configuration matrix on an empty table (cost model and gates), the default
configuration on the shipped table (exact entries, nearest-entry priors, the exact-float32 route) and on a hand-made
table that holds every kind of entry, and the key set and trial count of a tuning pass.  A change to that file is a
change of a launch decision: it has to be meant."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_route_chooses_what_the_manifest_records():
    """The tool runs in a child process (the switch that makes the library print its choices is read once, when the
    library first launches).  The trial count of the tuning pass follows from the candidate lists and the row lengths
    alone; two runs of the tool at the commit that recorded the manifest agreed on it, so it is compared as well."""
    with open(os.path.join(ROOT, "tests", "golden", "launch_routes.json")) as f:
        want = json.load(f)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dump_routes.py")], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-4000:]
    got = json.loads(res.stdout)
    assert sorted(got) == sorted(want)
    differing = [case for case in want if got[case] != want[case]]
    for case in differing[:5]:
        print(case, "\n  want", want[case], "\n  got ", got[case])
    assert not differing, differing
