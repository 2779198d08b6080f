// skx_unionfind.h -- the lock-free union-find of the device consumers of the pair sweep (skx_banded.hip: the clusters; skx_mst.hip: the rounds of
// the spanning forest), for .hip files only.  parent[x] <= x, a root has parent[x] == x.
// A link always points the HIGHER root at the LOWER one, by one 32-bit atomicMin on parent[higher].  Where the atomic finds that the higher
// node had been given a parent in the meantime it has still lowered that node's parent to min(old, lower), which keeps the node attached; what
// is left to join are the trees of `old` and `lower`, and the loop carries on with those two.  parent[] only ever decreases and parent[x] <= x,
// so no cycle can form and the root of a component is its lowest sample, whatever the order of the links.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace skx {

__device__ inline uint32_t uf_root(const uint32_t *parent, uint32_t x)
{
    for (uint32_t p; (p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x;) x = p;
    return x;
}
__device__ inline void uf_link(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = uf_root(parent, a); b = uf_root(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicMin(parent + hi, lo);
        if (old == hi) return;                    // hi was a root and now hangs under lo
        a = old; b = lo;                          // hi hangs under min(old, lo); the trees of old and lo are still to be joined
    }
}

}  // namespace skx
