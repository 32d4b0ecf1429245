// topo_paircmp.h -- device helpers of the kernels that compare a pair of tables (topo_diff.hip,
// topo_impact.hip) or of link loads (topo_shift.hip): the kind bits of one pair and the {largest
// rise, lowest index} merge of the count passes.  Device only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "topo_dev_common.h"

namespace shdtopo {
namespace dev {

// kind bits of pair (x0, h0) -> (x1, h1); 0: unchanged
__device__ __forceinline__ uint32_t pair_kind(const double2& x0, const double2& x1, uint32_t h0,
                                              uint32_t h1) {
    uint32_t k = 0;
    if (d2bits(x0.x) != d2bits(x1.x)) k |= x1.x > x0.x ? kDiffLatRose : (x1.x < x0.x ? kDiffLatFell : 0u);
    if (d2bits(x0.y) != d2bits(x1.y)) k |= kDiffRel;
    if (h0 != h1) k |= kDiffHops;
    return k;
}
__device__ __forceinline__ bool pair_changed(const double2& x0, const double2& x1, uint32_t h0,
                                             uint32_t h1) {
    return d2bits(x0.x) != d2bits(x1.x) || d2bits(x0.y) != d2bits(x1.y) || h0 != h1;
}

// Whether {r, c} replaces {rise, cur} as the {largest rise, lowest index reaching it}; an index
// below 0 holds no rise.  Symmetric, so every merge order ends with the same pair.  I: int32_t
// columns (the diff), int64_t flows (the impact) or entries (the load shift); R: the f64 latency
// rise of the first two, the u64 load and load difference of the shift.
template <class R, class I>
__device__ __forceinline__ bool worse_rise(R r, I c, R rise, I cur) {
    return c >= 0 && (cur < 0 || r > rise || (r == rise && c < cur));
}

// the wavefront's {largest rise, lowest index}, in every lane
template <class R, class I>
__device__ __forceinline__ void wave_worst_rise(R& rise, I& idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const R r = __shfl_xor(rise, o, 64);
        const I c = __shfl_xor(idx, o, 64);
        if (worse_rise(r, c, rise, idx)) {
            rise = r;
            idx = c;
        }
    }
}

}  // namespace dev
}  // namespace shdtopo
