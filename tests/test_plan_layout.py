"""CPU-tier: the host-side layout of every plan (2 nets x 4 precisions) is
exactly the one recorded in tests/golden/plan_layout.json -- parameter and
injection counts, pack and bias-blob sizes, workspace sizes and every
activation plane's offset and width at four sample counts.  The fixture was
recorded (tools/gen_plan_layout.py) from the build that preceded the plan
table, so it pins everything the table and the chain-set builder decide."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_layout_matches_the_recorded_fixture():
    import codenerf_amd._lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import gen_plan_layout as G
    want = json.load(open(G.FIXTURE))
    got = json.loads(json.dumps(G.record(L.load_library())))     # keys and tuples as JSON has them
    assert sorted(got) == sorted(want) and len(want) == 8
    for plan in want:
        assert got[plan] == want[plan], plan
