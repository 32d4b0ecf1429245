// topo_cross.hip -- link crossings for gfx950: which flows cross a set of watched links and routers.
//
// shdtopo_link_crossings (include/shd_topology_abi.h) reports, for the requested (source,
// destination, weight) flows, every hop of the route shdtopo_trace_routes reports that goes over a
// watched edge or arrives at a watched vertex -- link load's inverse question, answered like link
// load without writing a single route out.  The chains are the ones a trace and a load walk
// (topo_chain.h: the heap replay's vertex records or the batch slots' pair records), the hop
// counts and the broken-source protocol are link load's validation (topo_load.hip), and the
// staging of the records follows the trace (topo_trace.hip): chains die with their chunk, so
//
//   validate  launch_load_validate[_pairs]: hops[q], -1 when broken;
//   count     one thread per request walks destination -> source, bounded by hops[q], and tests
//             every hop's edge id and arrival vertex against the watch set; its record count goes
//             to lcnt[q] (chunk order) and gcnt[ridx] (request order), a hit adds 1 and the flow's
//             weight to the watch's totals;
//   scan      chunk-local exclusive scan of lcnt: the staging segments;
//   write     the same walk fills the request's segment from its end backwards, so the records
//             come out in route order (hop = hops - 1 - steps), the edge record of a hop before
//             its vertex record;
//   scatter   after the last chunk and the exclusive scan of gcnt: the segments of the flows that
//             end at or below the caller's cap are copied to the output at the call's offsets.
//
// The watch set is one bit per edge id and per relabelled vertex (1.25 MB + 125 KB at 10 M edges
// and 1 M vertices: it stays cache-resident next to the random record reads); only a hit searches
// the sorted id arrays for its watch index.  Hits are rare (a flow in a hundred), so the u64
// atomics on the watches' totals are not the hot addresses link load's accumulators were.  Sums are
// u64 and wrap: any order of the atomics gives the same result; everything else is a plain store
// into memory the call owns.
#include <hip/hip_runtime.h>

#include <algorithm>
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

// (the watch tests -- watch_find, edge_watch, vertex_watch -- are topo_watch.h's)
__device__ __forceinline__ void watch_add(const CrossWatch& cw, int32_t k, u64 w) {
    atomicAdd(&cw.wcount[k], 1ull);
    atomicAdd(&cw.wweight[k], w);
}

// PAIR: the chains are the batch slots' pair records (topo_chain.h).  EDGES: edges are watched --
// without them the pair form looks up no hop's replay-CSR entry (up<false>).
template <bool PAIR, bool EDGES>
__global__ void __launch_bounds__(kTB)
cross_count_kernel(ReplayCSR g, ReplayWs ws, PairChains pc, TraceIds ids, TraceReqs rq,
                   const u64* __restrict__ w, const int32_t* __restrict__ hops, CrossWatch cw,
                   int64_t* __restrict__ lcnt, int64_t* __restrict__ gcnt,
                   u64* __restrict__ cnt) {
    u64 nrec = 0, nflow = 0;
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        const uint32_t slot = rq.rslot[q], src = rq.rsrc[q], t = rq.rdst[q];
        Chain<PAIR> c;
        const int st = c.open(g, ws, pc, rq, slot, src, t);
        if (st == kChainSkip) continue;
        int64_t h = hops[q];
        int64_t n = 0;
        if (st == kChainOk && h >= 1) {
            const u64 wq = w[q];
            if (t == src) {
                int32_t k = EDGES ? edge_watch(cw, ids.selfEid[src]) : -1;
                if (k >= 0) {
                    watch_add(cw, k, wq);
                    n++;
                }
                k = vertex_watch(cw, src);
                if (k >= 0) {
                    watch_add(cw, k, wq);
                    n++;
                }
            } else {
                uint32_t v = t;
                while (v != src && h-- > 0) {  // (the validation counted h hops)
                    uint32_t p = 0, j = 0;
                    if (!c.template up<EDGES>(g, ids, v, p, j)) break;
                    int32_t k = EDGES ? edge_watch(cw, ids.eid[j]) : -1;
                    if (k >= 0) {
                        watch_add(cw, k, wq);
                        n++;
                    }
                    k = vertex_watch(cw, v);
                    if (k >= 0) {
                        watch_add(cw, k, wq);
                        n++;
                    }
                    v = p;
                }
            }
        }
        lcnt[q] = n;
        gcnt[rq.ridx[q]] = n;
        nrec += (u64)n;
        nflow += n > 0;
    }
    // every lane reaches this point: one atomic per wavefront and counter
    nrec = wave_sum_u64(nrec);
    nflow = wave_sum_u64(nflow);
    if ((threadIdx.x & 63) == 0) {
        if (nrec) atomicAdd(&cnt[CR_RECORDS], nrec);
        if (nflow) atomicAdd(&cnt[CR_FLOWS], nflow);
    }
}

template <bool PAIR, bool EDGES>
__global__ void __launch_bounds__(kTB)
cross_write_kernel(ReplayCSR g, ReplayWs ws, PairChains pc, TraceIds ids, TraceReqs rq,
                   const int32_t* __restrict__ hops, CrossWatch cw,
                   const int64_t* __restrict__ loff, CrossRec* __restrict__ stage) {
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        const uint32_t slot = rq.rslot[q], src = rq.rsrc[q], t = rq.rdst[q];
        Chain<PAIR> c;
        if (c.open(g, ws, pc, rq, slot, src, t) != kChainOk) continue;
        const int64_t h = hops[q];
        const int64_t base = loff[q];
        int64_t pos = loff[q + 1];  // the segment is filled from its end; never below base
        if (h < 1 || pos <= base) continue;
        const int32_t flow = (int32_t)rq.ridx[q];
        if (t == src) {
            int32_t k = vertex_watch(cw, src);
            if (k >= 0 && pos > base) stage[--pos] = CrossRec{flow, k, 0, 0};
            k = EDGES ? edge_watch(cw, ids.selfEid[src]) : -1;
            if (k >= 0 && pos > base) stage[--pos] = CrossRec{flow, k, 0, 0};
            continue;
        }
        uint32_t v = t;
        for (int64_t hop = h - 1; hop >= 0 && v != src && pos > base; --hop) {
            uint32_t p = 0, j = 0;
            if (!c.template up<EDGES>(g, ids, v, p, j)) break;  // (the validation walked the chain)
            int32_t k = vertex_watch(cw, v);
            if (k >= 0) stage[--pos] = CrossRec{flow, k, (int32_t)hop, 0};
            if (EDGES && pos > base) {
                const int32_t e = ids.eid[j];
                k = edge_watch(cw, e);
                if (k >= 0) stage[--pos] = CrossRec{flow, k, (int32_t)hop, ids.perm[p] != cw.eu[e]};
            }
            v = p;
        }
    }
}

__global__ void __launch_bounds__(kTB)
cross_scatter_kernel(TraceReqs rq, const int64_t* __restrict__ goff,
                     const int64_t* __restrict__ loff, const CrossRec* __restrict__ stage,
                     CrossRec* __restrict__ out, int64_t cap) {
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        const uint32_t i = rq.ridx[q];
        const int64_t o = goff[i], end = goff[i + 1];
        if (end <= o || end > cap) continue;
        const int64_t base = loff[q];
        for (int64_t k = 0; k < end - o; ++k) out[o + k] = stage[base + k];
    }
}

bool watch_ok(const CrossWatch& cw) {
    return cw.ebits && cw.vbits && cw.wcount && cw.wweight && cw.ne >= 0 && cw.nv >= 0 &&
           (cw.ne == 0 || (cw.eids && cw.eidx && cw.eu)) && (cw.nv == 0 || (cw.vids && cw.vidx));
}
bool pairs_ok(const PairChains& pc, const TraceReqs& rq) {
    return rq.rmap && pc.prec && pc.counters && pc.kf >= 1 && pc.kf <= pc.K;
}

}  // namespace

hipError_t launch_cross_count(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                              const TraceReqs& rq, const unsigned long long* w,
                              const int32_t* hops, const CrossWatch& cw, int64_t* lcnt,
                              int64_t* gcnt, unsigned long long* cnt, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!watch_ok(cw)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((cross_count_kernel<false, true>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                       stream, g, ws, PairChains{}, ids, rq, w, hops, cw, lcnt, gcnt, cnt);
    return hipGetLastError();
}

hipError_t launch_cross_write(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                              const TraceReqs& rq, const int32_t* hops, const CrossWatch& cw,
                              const int64_t* loff, CrossRec* stage, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!watch_ok(cw)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((cross_write_kernel<false, true>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                       stream, g, ws, PairChains{}, ids, rq, hops, cw, loff, stage);
    return hipGetLastError();
}

hipError_t launch_cross_count_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                    const TraceReqs& rq, const unsigned long long* w,
                                    const int32_t* hops, const CrossWatch& cw, int64_t* lcnt,
                                    int64_t* gcnt, unsigned long long* cnt, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!watch_ok(cw) || !pairs_ok(pc, rq)) return hipErrorInvalidValue;
    if (cw.ne > 0)
        hipLaunchKernelGGL((cross_count_kernel<true, true>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                           stream, g, ReplayWs{}, pc, ids, rq, w, hops, cw, lcnt, gcnt, cnt);
    else
        hipLaunchKernelGGL((cross_count_kernel<true, false>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                           stream, g, ReplayWs{}, pc, ids, rq, w, hops, cw, lcnt, gcnt, cnt);
    return hipGetLastError();
}

hipError_t launch_cross_write_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                    const TraceReqs& rq, const int32_t* hops, const CrossWatch& cw,
                                    const int64_t* loff, CrossRec* stage, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!watch_ok(cw) || !pairs_ok(pc, rq)) return hipErrorInvalidValue;
    if (cw.ne > 0)
        hipLaunchKernelGGL((cross_write_kernel<true, true>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                           stream, g, ReplayWs{}, pc, ids, rq, hops, cw, loff, stage);
    else
        hipLaunchKernelGGL((cross_write_kernel<true, false>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                           stream, g, ReplayWs{}, pc, ids, rq, hops, cw, loff, stage);
    return hipGetLastError();
}

hipError_t launch_cross_scatter(const TraceReqs& rq, const int64_t* goff, const int64_t* loff,
                                const CrossRec* stage, CrossRec* out, int64_t cap,
                                hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cross_scatter_kernel, dim3(grid_for(rq.n)), dim3(kTB), 0, stream, rq, goff,
                       loff, stage, out, cap);
    return hipGetLastError();
}

}  // namespace shdtopo
