"""-m gpu: examples/shortcut_constrained.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_shortcut_constrained_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "shortcut_constrained.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    # what holds by construction: a plan, a shortcut of status 0 that keeps the constraint and is not blocked
    m = re.search(r"^plan_rrt_constrained: status 0, (\d+) waypoints, length [\d.]+ rad$", res.stdout, re.M)
    assert m and 3 <= int(m.group(1)) <= 64, res.stdout
    s = re.search(r"^shortcut_paths_constrained: status 0, (\d+) waypoints, length [\d.]+ rad \(input [\d.]+ rad\); "
                  r"(\d+) projections, (\d+) ended on the constraint$", res.stdout, re.M)
    assert s and 2 <= int(s.group(1)) <= 32 and int(s.group(2)) >= int(s.group(3)), res.stdout
    assert re.search(r"^  constraint kept \(violation [\d.]+\); certified (free|undecided)$", res.stdout, re.M), res.stdout
    # what is printed and not judged: the resampled path's two checks and the timing at the URDF's limits
    assert re.search(r"^resample_paths_constrained: status [04], 32 waypoints, \d+ of 30 projected; new segments free: "
                     r"(True|False), on the constraint: (True|False)$", res.stdout, re.M), res.stdout
    assert len(re.findall(r"^  timed at the URDF's velocity limits: status \d, (nan|[\d.]+) s$", res.stdout, re.M)) == 2, \
        res.stdout
