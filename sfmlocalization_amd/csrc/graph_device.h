// Connected components of an edge list on the device: what tracks.hip (nodes = feature rows, edges = matches) and
// globalposes.hip (nodes = views, edges = the pairs that carry a translation) share.  parent[x] <= x always: a pass
// hooks, for every edge whose ends have different roots, the larger root under the smaller one (atomicMin on the root's
// parent, an integer minimum: the same whatever the order), then every node jumps to its root.  Passes repeat until one
// hooks nothing; then every edge has both ends under one root and a root is the smallest node of its component.  The
// fixed point does not depend on scheduling; only the number of passes does, and nothing reports it.  An edge whose two
// ends are the same node hooks nothing: that is how a caller masks an edge out.  Everything is in the anonymous
// namespace: each translation unit compiles its own copy, no device symbol crosses one.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sfmloc {
namespace {

// the root of x; parent[] descends strictly until it, whatever other lanes hook meanwhile
__device__ __forceinline__ uint32_t graph_find(const uint32_t *parent, uint32_t x) {
  for (;;) {
    const uint32_t p = __atomic_load_n(parent + x, __ATOMIC_RELAXED);
    if (p == x) return x;
    x = p;
  }
}

// hook.  A root that another lane hooks at the same time keeps the smaller of the two parents; the edge that lost is
// met again in the next pass, which is why the loop ends on a pass without a hook.
__global__ __launch_bounds__(256) void k_graph_hook(const uint32_t *__restrict__ ea, const uint32_t *__restrict__ eb,
                                                    uint32_t m, uint32_t *parent, uint32_t *changed) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= m) return;
  const uint32_t ra = graph_find(parent, ea[e]), rb = graph_find(parent, eb[e]);
  if (ra == rb) return;
  atomicMin(parent + (ra > rb ? ra : rb), ra > rb ? rb : ra);
  *changed = 1;
}

// pointer jumping, all the way (no hook runs beside it: the roots stand still)
__global__ __launch_bounds__(256) void k_graph_jump(uint32_t *parent, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = graph_find(parent, i);
  __atomic_store_n(parent + i, r, __ATOMIC_RELAXED);
}

}  // namespace
}  // namespace sfmloc
