"""-m gpu: examples/motion_certify.py runs on the Panda and shows what it is there to show."""
import os
import subprocess
import sys

import pytest

from conftest import ROBOTS, ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def test_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "motion_certify.py"),
                          os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    assert "the samples stepped over the plate: True" in res.stdout, res.stdout
    assert "certified, tol 0.001 m: blocked" in res.stdout and "plan:" in res.stdout, res.stdout
