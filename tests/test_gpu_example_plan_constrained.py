"""-m gpu: examples/plan_constrained.py runs as a user would run it, with a small roadmap."""
import os
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_plan_constrained_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "plan_constrained.py"), *PANDA, "256"], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    assert "constrained roadmap:" in res.stdout and "unconstrained plan:" in res.stdout, res.stdout
    assert "constrained plan: found" in res.stdout and "constraint kept" in res.stdout, res.stdout
