// ik_grid.hpp -- the grid of a grid-stride launch: stride_grid, plain C++ (the one place).
//
// A row kernel strides over its work, so its grid only has to be large enough to fill the device: the blocks the work
// needs, at most `device_cap` of them.  The option grid_cap (ik_host.hpp: Options) puts its own number in the place of
// the device's, so that a test takes the second and later trips of a kernel's loop with a few hundred rows instead of
// the half million a full device asks for.  No result depends on the grid.
#pragma once

namespace optik {
namespace host {

// Blocks for `work` items at `block` items per block: at least 1, at most the cap -- grid_cap when it is >= 1,
// device_cap otherwise.
inline int stride_grid(unsigned long long work, int block, long long device_cap, int grid_cap) {
    unsigned long long blocks = work / (unsigned long long)block + (work % (unsigned long long)block ? 1 : 0);
    long long cap = grid_cap >= 1 ? (long long)grid_cap : device_cap;
    if (cap > 0x7fffffffll) cap = 0x7fffffffll;
    if (cap < 1) cap = 1;
    if (blocks > (unsigned long long)cap) blocks = (unsigned long long)cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

}  // namespace host
}  // namespace optik
