"""examples/amg_elasticity_beam.py runs at its toy size: both recipes converge to the same field, and the rigid-body modes take fewer linear iterations."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_the_beam_example_runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "amg_elasticity_beam.py")], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    print(rec)
    assert rec["converged"] and rec["max_relative_difference"] <= 1e-6
    assert len(rec["rigid_body"]["levels"]) >= 2 and rec["rigid_body"]["levels"][-1] <= 32
    assert sum(rec["rigid_body"]["linear_iterations"]) < sum(rec["translations"]["linear_iterations"])
