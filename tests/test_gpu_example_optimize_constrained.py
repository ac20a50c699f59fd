"""-m gpu: examples/optimize_constrained.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]
NUM = r"(nan|inf|-?[\d.]+(?:e[-+]\d+)?)"


def test_optimize_constrained_example():
    from optik_amd import _native as nat
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "optimize_constrained.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    assert re.search(r"^plan_rrt_constrained: status 0, \d+ waypoints$", res.stdout, re.M), res.stdout
    before = re.search(rf"^before: clearance {NUM} m, violation {NUM}$", res.stdout, re.M)
    after = re.search(rf"^after: clearance {NUM} m, violation {NUM}$", res.stdout, re.M)
    assert before and after, res.stdout
    # what holds by construction: the waypoints of the result are on the constraint at ptol where the input's were
    assert float(before.group(2)) <= nat.CONSTRAINT_TOL, "the resampled path's waypoints are projected"
    assert float(after.group(2)) <= nat.CONSTRAINT_TOL, res.stdout
    s = re.search(r"^optimize_paths_constrained: status 0, .*; (\d+) projections, (\d+) ended on the constraint; "
                  r"segments free: (True|False), on the constraint: (True|False)$", res.stdout, re.M)
    assert s and int(s.group(1)) >= int(s.group(2)) > 0, res.stdout
    # printed and not judged: the clearance, the costs, the two checks of the segments, the timing
    assert re.search(r"^  timed at the URDF's velocity limits: status \d, (nan|[\d.]+) s$", res.stdout, re.M), res.stdout
