"""MI355X: the captured step of LatentInverter with its optional parts (fit_parts: landmark term, region, camera; and the
shared identity) has the kernel nodes it had before the parts were split out of the inverter.  The counts in
tests/golden/inverter_nodes_parent.json were written by scripts/record_inverter.py on the commit the file names, on the
same tiny problem; a part that launches once more or once less, or in another place, shows here."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import record_inverter  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "inverter_nodes_parent.json")) as _f:
    PARENT = json.load(_f)


@pytest.mark.parametrize("number", [3, 5, 6, 7, 9])
def test_captured_step_has_the_parent_commits_kernel_nodes(number):
    name = record_inverter.CONFIGS[number][0]
    inv = record_inverter.make(number, "cuda", True)[0]
    hist = inv.run(record_inverter.STEPS)
    assert inv.graph is not None and bool(torch.isfinite(hist).all())
    print("%s: %d kernel nodes, %d at %s" % (name, inv.graph.kernel_nodes, PARENT["kernel_nodes"][name],
                                             PARENT["recorded_at_commit"]))
    assert inv.graph.kernel_nodes == PARENT["kernel_nodes"][name]
