// topo_timeline.hip -- link timeline for gfx950: per-time-bin traffic on watched links and routers.
//
// shdtopo_link_timeline (include/shd_topology_abi.h) bins, for the requested (source, destination,
// weight, emission time) flows, every hop of the route shdtopo_trace_routes reports that goes over
// a watched edge or arrives at a watched vertex by the time the flow reaches it: the emission time
// plus the latency of the route's prefix.  The chains, the hop counts and the broken-source
// protocol are the crossings' (topo_chain.h, launch_load_validate[_pairs]), the watch tests too
// (topo_watch.h).  What differs is the direction: a chain is walked destination -> source, a
// prefix latency is summed source -> hop by one IEEE add per hop (the trace's pass 2), so a flow
// with a hit parks its hops in HBM and runs over them once more, front to back:
//
//   validate  launch_load_validate[_pairs]: hops[q], -1 when broken;
//   mark      one thread per request walks destination -> source, bounded by hops[q], and tests
//             every hop's edge id and arrival vertex against the watch bitmaps: seg[q] = hops[q]
//             when the flow has a hit, else 0 -- a flow without a hit costs this one walk;
//   scan      chunk-local exclusive scan of seg: the staging segments of the flows with a hit;
//   time      the same walk parks {replay-CSR entry, arrival vertex} of hop k at segment position
//             k (8 B a hop, filled back to front), then runs front to back: the latency by
//             __dadd_rn from 0.0, the watch tests again, one u64 atomicAdd per hit into the call's
//             bins.  A self pair is its loop: no staging.
//
// A route of any length is a longer segment.  The bins are u64[rows x nbins] followed by the
// `outside` pairs u64[rows x 2] (rows = 2 ne + nv), zeroed by the caller per call and copied out
// once.  Sums are u64 and wrap: any order of the atomics gives the same result; everything else
// is a plain store into memory the call owns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "topo_chain.h"
#include "topo_watch.h"

namespace shdtopo {

namespace {

using namespace dev;
using u64 = unsigned long long;

constexpr int kTB = 256;

__device__ __forceinline__ int64_t gtid() {
    return (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
}
__device__ __forceinline__ int64_t gstride() { return (int64_t)gridDim.x * blockDim.x; }
unsigned grid_for(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kTB - 1) / kTB, 65536));
}

// the packet kernel's conversion (topo_kernels.hip): milliseconds -> nanoseconds, rounded up
__device__ __forceinline__ u64 lat_ns(double ms) { return (u64)ceil(ms * 1000000.0); }

// hit counters of one thread, summed per wavefront at the kernel's end
struct HitCount {
    u64 in = 0, before = 0, after = 0;
};
// weight w of a hit of row `row` at time t
__device__ __forceinline__ void bin_add(const TimeBins& tb, int64_t row, u64 t, u64 w,
                                        HitCount& hc) {
    if ((uint64_t)row >= (uint64_t)tb.rows) return;  // (the watch indices are below rows)
    u64* outside = tb.acc + tb.rows * tb.nbins + 2 * row;
    if (t < tb.t0) {
        atomicAdd(&outside[0], w);
        hc.before++;
        return;
    }
    if (tb.nbins > 0) {  // (binNs > 0 then)
        const u64 b = (t - tb.t0) / tb.binNs;
        if (b < (u64)tb.nbins) {
            atomicAdd(&tb.acc[row * tb.nbins + (int64_t)b], w);
            hc.in++;
            return;
        }
    }
    atomicAdd(&outside[1], w);
    hc.after++;
}

// PAIR: the chains are the batch slots' pair records (topo_chain.h).  EDGES: edges are watched --
// without them the pair form's mark walk looks up no hop's replay-CSR entry (up<false>).
template <bool PAIR, bool EDGES>
__global__ void __launch_bounds__(kTB)
timeline_mark_kernel(ReplayCSR g, ReplayWs ws, PairChains pc, TraceIds ids, TraceReqs rq,
                     const int32_t* __restrict__ hops, CrossWatch cw, int64_t* __restrict__ seg,
                     u64* __restrict__ cnt) {
    u64 nflow = 0, nstage = 0;
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        const uint32_t slot = rq.rslot[q], src = rq.rsrc[q], t = rq.rdst[q];
        Chain<PAIR> c;
        const int st = c.open(g, ws, pc, rq, slot, src, t);
        if (st == kChainSkip) continue;
        const int64_t h = hops[q];
        bool hit = false;
        if (st == kChainOk && h >= 1) {
            if (t == src) {
                hit = (EDGES && edge_watch(cw, ids.selfEid[src]) >= 0) ||
                      vertex_watch(cw, src) >= 0;
            } else {
                uint32_t v = t;
                int64_t left = h;
                while (!hit && v != src && left-- > 0) {  // (the validation counted h hops)
                    uint32_t p = 0, j = 0;
                    if (!c.template up<EDGES>(g, ids, v, p, j)) break;
                    hit = (EDGES && edge_watch(cw, ids.eid[j]) >= 0) || vertex_watch(cw, v) >= 0;
                    v = p;
                }
            }
        }
        seg[q] = hit ? h : 0;
        nflow += hit;
        if (hit && t != src) nstage += (u64)h;
    }
    // every lane reaches this point: one atomic per wavefront and counter
    nflow = wave_sum_u64(nflow);
    nstage = wave_sum_u64(nstage);
    if ((threadIdx.x & 63) == 0) {
        if (nflow) atomicAdd(&cnt[TL_FLOWS], nflow);
        if (nstage) atomicAdd(&cnt[TL_STAGED], nstage);
    }
}

template <bool PAIR, bool EDGES>
__global__ void __launch_bounds__(kTB)
timeline_time_kernel(ReplayCSR g, ReplayWs ws, PairChains pc, TraceIds ids, TraceReqs rq,
                     const u64* __restrict__ w, const u64* __restrict__ now,
                     const int32_t* __restrict__ hops, CrossWatch cw,
                     const int64_t* __restrict__ loff, uint2* __restrict__ stage, TimeBins tb,
                     u64* __restrict__ cnt) {
    HitCount hc;
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        const uint32_t slot = rq.rslot[q], src = rq.rsrc[q], t = rq.rdst[q];
        Chain<PAIR> c;
        if (c.open(g, ws, pc, rq, slot, src, t) != kChainOk) continue;
        const int64_t h = hops[q];
        const int64_t base = loff[q];
        if (h < 1 || loff[q + 1] - base != h) continue;  // no hit: no segment
        const u64 wq = w[q], tq = now[q];
        if (t == src) {
            // the self loop: entered at the emission time, arrival after its latency
            int32_t k = EDGES ? edge_watch(cw, ids.selfEid[src]) : -1;
            if (k >= 0) bin_add(tb, k, tq, wq, hc);
            k = vertex_watch(cw, src);
            if (k >= 0) bin_add(tb, (int64_t)cw.ne + k, tq + lat_ns(0.0 + g.selfLat[src]), wq, hc);
            continue;
        }
        // back to front: hop k of the route (vertex k -> k + 1) at base + k
        uint32_t v = t;
        int64_t k = h;
        while (k > 0 && v != src) {
            uint32_t p = 0, j = 0;
            if (!c.template up<true>(g, ids, v, p, j)) break;  // (the validation walked the chain)
            stage[base + --k] = make_uint2(j, v);
            v = p;
        }
        if (k != 0 || v != src) continue;
        // front to back: the helper's order, one IEEE add per hop from the source
        double lat = 0.0;
        uint32_t a = src;
        for (k = 0; k < h; ++k) {
            const uint2 s = stage[base + k];
            if ((int64_t)s.x >= g.nadj) break;
            const u64 enter = tq + lat_ns(lat);
            lat = __dadd_rn(lat, g.hop[s.x].x);
            if (EDGES) {
                const int32_t e = ids.eid[s.x];
                const int32_t ke = edge_watch(cw, e);
                if (ke >= 0)  // the forward rows first, then the reverse rows (a != eu[e])
                    bin_add(tb, ids.perm[a] != cw.eu[e] ? (int64_t)cw.ne + ke : (int64_t)ke, enter,
                            wq, hc);
            }
            const int32_t kv = vertex_watch(cw, s.y);
            if (kv >= 0) bin_add(tb, (int64_t)cw.ne + kv, tq + lat_ns(lat), wq, hc);
            a = s.y;
        }
    }
    // every lane reaches this point: one atomic per wavefront and counter
    const u64 nin = wave_sum_u64(hc.in), nbef = wave_sum_u64(hc.before),
              naft = wave_sum_u64(hc.after);
    if ((threadIdx.x & 63) == 0) {
        if (nin) atomicAdd(&cnt[TL_IN], nin);
        if (nbef) atomicAdd(&cnt[TL_BEFORE], nbef);
        if (naft) atomicAdd(&cnt[TL_AFTER], naft);
    }
}

bool watch_ok(const CrossWatch& cw) {
    return cw.ebits && cw.vbits && cw.ne >= 0 && cw.nv >= 0 &&
           (cw.ne == 0 || (cw.eids && cw.eidx && cw.eu)) && (cw.nv == 0 || (cw.vids && cw.vidx));
}
bool pairs_ok(const PairChains& pc, const TraceReqs& rq) {
    return rq.rmap && pc.prec && pc.counters && pc.kf >= 1 && pc.kf <= pc.K;
}
bool bins_ok(const TimeBins& tb, const CrossWatch& cw) {
    return tb.acc && tb.nbins >= 0 && tb.rows == 2 * (int64_t)cw.ne + cw.nv &&
           (tb.nbins == 0 || tb.binNs > 0);
}

}  // namespace

hipError_t launch_timeline_mark(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                                const TraceReqs& rq, const int32_t* hops, const CrossWatch& cw,
                                int64_t* seg, unsigned long long* cnt, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!watch_ok(cw)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((timeline_mark_kernel<false, true>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                       stream, g, ws, PairChains{}, ids, rq, hops, cw, seg, cnt);
    return hipGetLastError();
}

hipError_t launch_timeline_time(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                                const TraceReqs& rq, const unsigned long long* w,
                                const unsigned long long* now, const int32_t* hops,
                                const CrossWatch& cw, const int64_t* loff, uint2* stage,
                                const TimeBins& tb, unsigned long long* cnt, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!watch_ok(cw) || !bins_ok(tb, cw)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((timeline_time_kernel<false, true>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                       stream, g, ws, PairChains{}, ids, rq, w, now, hops, cw, loff, stage, tb, cnt);
    return hipGetLastError();
}

hipError_t launch_timeline_mark_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                      const TraceReqs& rq, const int32_t* hops,
                                      const CrossWatch& cw, int64_t* seg, unsigned long long* cnt,
                                      hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!watch_ok(cw) || !pairs_ok(pc, rq)) return hipErrorInvalidValue;
    if (cw.ne > 0)
        hipLaunchKernelGGL((timeline_mark_kernel<true, true>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                           stream, g, ReplayWs{}, pc, ids, rq, hops, cw, seg, cnt);
    else
        hipLaunchKernelGGL((timeline_mark_kernel<true, false>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                           stream, g, ReplayWs{}, pc, ids, rq, hops, cw, seg, cnt);
    return hipGetLastError();
}

hipError_t launch_timeline_time_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                      const TraceReqs& rq, const unsigned long long* w,
                                      const unsigned long long* now, const int32_t* hops,
                                      const CrossWatch& cw, const int64_t* loff, uint2* stage,
                                      const TimeBins& tb, unsigned long long* cnt,
                                      hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!watch_ok(cw) || !pairs_ok(pc, rq) || !bins_ok(tb, cw)) return hipErrorInvalidValue;
    if (cw.ne > 0)
        hipLaunchKernelGGL((timeline_time_kernel<true, true>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                           stream, g, ReplayWs{}, pc, ids, rq, w, now, hops, cw, loff, stage, tb,
                           cnt);
    else
        hipLaunchKernelGGL((timeline_time_kernel<true, false>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                           stream, g, ReplayWs{}, pc, ids, rq, w, now, hops, cw, loff, stage, tb,
                           cnt);
    return hipGetLastError();
}

}  // namespace shdtopo
