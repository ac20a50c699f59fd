"""-m gpu: examples/ik_repair.py runs as a user would run it."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROBOTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANDA = [os.path.join(ROBOTS, "panda.urdf"), "panda_link0", "panda_link8"]


def test_ik_repair_example():
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ik_repair.py"), *PANDA], env=env,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    # the story: the start inside the table is refused, pushed out by a few hundredths of a radian, and then planned
    m = re.search(r"^start: clearance (-[\d.]+) mm; plan_rrt: status (\d+)$", res.stdout, re.M)
    assert m and -10.0 < float(m.group(1)) < 0.0 and int(m.group(2)) != 0, res.stdout
    m = re.search(r"^repaired: status 0 after (\d+) steps, moved ([\d.]+) rad, clearance ([\d.]+) mm$", res.stdout, re.M)
    assert m and 1 <= int(m.group(1)) <= 256 and float(m.group(2)) < 0.1 and float(m.group(3)) >= 20.0, res.stdout
    assert re.search(r"^plan_rrt from the repaired start: status 0, \d+ waypoints$", res.stdout, re.M), res.stdout
    m = re.search(r"^tool held within 20 mm: status 0 after (\d+) steps, moved [\d.]+ rad, clearance ([\d.]+) mm, "
                  r"violation ([\d.e+-]+)$", res.stdout, re.M)
    assert m and float(m.group(2)) >= 20.0 and float(m.group(3)) <= 1e-6, res.stdout
    m = re.search(r"^cell: (\d+) of 256 configurations closer than 20 mm; (\d+) repaired", res.stdout, re.M)
    assert m and int(m.group(1)) >= 32 and int(m.group(2)) >= 0.85 * int(m.group(1)), res.stdout
    m = re.search(r"^tool held within 1 mm: status 1 after 256 steps, moved [\d.]+ rad, clearance (-[\d.]+) mm", res.stdout,
                  re.M)
    assert m and -5.0 < float(m.group(1)) < 0.0, res.stdout
    # ik_region low over the table: repair gives more configurations from the same restarts, all free and in region
    rows = re.findall(r"^ik_region \d: (\d+) configurations without repair, (\d+) with \((\d+) of 16 restarts repaired\); "
                      r"smallest clearance ([\d.]+) mm, largest violation ([\d.e+-]+)$", res.stdout, re.M)
    assert len(rows) == 2, res.stdout
    for without, with_, repaired, clr, v in rows:
        assert int(with_) > int(without) >= 1 and int(repaired) >= 4 and float(clr) >= 0.0 and float(v) <= 1e-6, res.stdout
