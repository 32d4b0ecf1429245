// topo_watch.h -- the watch tests of the route walks (topo_cross.hip, topo_timeline.hip).
//
// A CrossWatch (topo_device.h) holds one bit per edge id and per relabelled vertex for the per-hop
// test; only a hit searches the sorted id arrays for its watch index (edges k, vertices ne + k).
#pragma once

#include "topo_device.h"

namespace shdtopo {
namespace dev {

// position of x in the ascending ids[0..n), -1 when absent
__device__ __forceinline__ int32_t watch_find(const int32_t* __restrict__ ids, int32_t n,
                                              int32_t x) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const int32_t y = ids[mid];
        if (y == x) return mid;
        if (y < x) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}
// watch index of edge e / relabelled vertex v, -1 when not watched (or e is no edge)
__device__ __forceinline__ int32_t edge_watch(const CrossWatch& cw, int32_t e) {
    if ((uint32_t)e >= (uint64_t)cw.E) return -1;
    if (!((cw.ebits[(uint32_t)e >> 5] >> (e & 31)) & 1u)) return -1;
    const int32_t i = watch_find(cw.eids, cw.ne, e);
    return i < 0 ? -1 : cw.eidx[i];
}
__device__ __forceinline__ int32_t vertex_watch(const CrossWatch& cw, uint32_t v) {
    if (!((cw.vbits[v >> 5] >> (v & 31)) & 1u)) return -1;
    const int32_t i = watch_find(cw.vids, cw.nv, (int32_t)v);
    return i < 0 ? -1 : cw.vidx[i];
}

}  // namespace dev
}  // namespace shdtopo
