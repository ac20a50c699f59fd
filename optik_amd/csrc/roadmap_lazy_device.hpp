// roadmap_lazy_device.hpp -- what the two lazy loops share on the device side (ik_roadmap_lazy.hip defines it;
// ik_roadmap_goals_lazy.hip uses it): the chain's lazy workspace, the reset from node flags, and the check of a
// round's claimed slots.
#pragma once

#include "collision_device.hpp"
#include "roadmap_lazy_measure.hpp"

namespace optik {
namespace lazydev {

constexpr int LAZY_BLOCK = 256;

inline unsigned blocks(long long work) { return (unsigned)((work + LAZY_BLOCK - 1) / LAZY_BLOCK); }
inline size_t align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

struct GraphArgs {
    const double *nodes;
    int32_t N, k;
    const int32_t *nbr;
    double *w0, *w;
    int32_t *verdict;
};

// the chain's lazy workspace, at least `bytes` (grown on demand, as optik_hip_roadmap_edges grows its own)
int reserve_ws(optik_hip_chain *ch, size_t bytes, unsigned char **out);

// rule 2 of roadmap_lazy_measure.hpp on the stream; d_node_free null: the nodes are classified first
int reset_launch(optik_hip_chain *ch, const double *ee_offset7, const GraphArgs &g, int lengths,
                 const uint8_t *d_node_free, hipStream_t stream);

// rule 4 of roadmap_lazy_measure.hpp for the `count` slots of d_list: their segments are gathered into d_qa
// ([2][n][count]) and checked at `resolution` into d_free [count], then marked; with d_edge_free [k][N] not null it
// stands for the motion check and d_free, d_qa are not touched.
int check_claimed(optik_hip_chain *ch, const double *ee_offset7, const GraphArgs &g, double resolution,
                  const uint8_t *d_edge_free, const int32_t *d_list, int32_t count, unsigned char *d_free,
                  double *d_qa, hipStream_t stream);

}  // namespace lazydev
}  // namespace optik
