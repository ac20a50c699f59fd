"""The grid of a grid-stride launch (optik_amd/csrc/ik_grid.hpp: stride_grid) as a pure function, compiled with g++: the
blocks the work needs, at most the device's cap or, when it is set, the option grid_cap -- no GPU.
tests/test_gpu_grid_stride.py runs the kernels under such grids."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "optik_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include "ik_grid.hpp"

// one line per query: work block device_cap grid_cap -> blocks
int main() {
    unsigned long long work;
    long long block, device_cap, grid_cap;
    while (std::scanf("%llu %lld %lld %lld", &work, &block, &device_cap, &grid_cap) == 4)
        std::printf("%d\n", optik::host::stride_grid(work, (int)block, device_cap, (int)grid_cap));
    return 0;
}
"""


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile ik_grid.hpp on its own"
    d = tmp_path_factory.mktemp("stride_grid")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(queries):
        text = "".join(" ".join(str(int(v)) for v in q) + "\n" for q in queries)
        res = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True)
        out = [int(ln) for ln in res.stdout.split()]
        assert len(out) == len(queries)
        return out
    return run


HUGE = 2 ** 43  # the item bound of the largest motion launch: 2^30 segments of up to 4097 samples
DEVICE = 256 * 8  # 8 blocks per CU on 256 CUs


def test_blocks_for_work_and_cap(grid):
    #        work, cap 0 (the device's), cap 1, cap 3
    table = [(0, 1, 1, 1), (1, 1, 1, 1), (256, 1, 1, 1), (257, 2, 1, 2), (512, 2, 1, 2), (513, 3, 1, 3),
             (805, 4, 1, 3), (DEVICE * 256, DEVICE, 1, 3), (DEVICE * 256 + 1, DEVICE, 1, 3), (HUGE, DEVICE, 1, 3),
             (2 ** 64 - 1, DEVICE, 1, 3)]
    queries = [(work, 256, DEVICE, cap) for work, *_ in table for cap in (0, 1, 3)]
    want = [b for _, *blocks in table for b in blocks]
    assert grid(queries) == want


def test_the_option_takes_the_devices_place_and_other_block_sizes(grid):
    # a cap above the device's is honoured too (the option replaces the device's number, it is not a second minimum)
    assert grid([(10 ** 9, 256, DEVICE, 5000)]) == [5000]
    # trajectory_sample: 2^20 blocks unless the option says otherwise
    assert grid([(2 ** 40, 256, 2 ** 20, 0), (2 ** 40, 256, 2 ** 20, 1), (805, 256, 2 ** 20, 0)]) == [2 ** 20, 1, 4]
    # path_optimize: 4 paths of 64 lanes per block
    assert grid([(11 * 64, 256, DEVICE, 0), (11 * 64, 256, DEVICE, 1), (11 * 64, 256, DEVICE, 3)]) == [3, 1, 3]
    # a device that reports nothing useful still launches one block; the result always fits an int
    assert grid([(805, 256, 0, 0), (805, 256, -4, 0), (2 ** 63, 1, 2 ** 40, 0)]) == [1, 1, 2 ** 31 - 1]
