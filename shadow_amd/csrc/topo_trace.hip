// topo_trace.hip -- route tracing for gfx950: the vertex / edge path behind a table entry.
//
// The reference's per-target helper (shd-topology.c:561-671) walks a vertex list, sums the
// igraph_get_eid edge latencies and multiplies the reliabilities; at debug level it logs the path
// (:594,644,654-656).  The table kernels walk the same chains and keep {lat, rel, hops} only.
// Here the chains are written out: the heap replay (topo_replay.hip, its trace launch) leaves
// igraph's parent of every popped vertex in the slot's vertex records, and route_trace_kernel
// walks them for the requested (source, destination) pairs.  A source whose row the batch kernel's
// keep launch (topo_sssp_batch.hip) leaves unflagged needs no replay: the same walk runs over the
// batch slot's pair records instead (route_trace_kernel<PASS, true>; topo_chain.h has the two
// chain sources), finding each hop's replay-CSR entry by a binary search of the parent's row.
//
//   pass 1  one thread per request walks destination -> source and counts the hops, with the
//           replay epilogue's guards (unreached vertex, slot out of range, more than V hops);
//   scan    device exclusive scans of hops + 1: per chunk (staging positions) and, once every
//           chunk is walked, in request order (the call's offsets);
//   pass 2  the same walk writes the route back to front into the chunk's staging arrays (a
//           route of any length is just a longer walk: the output is in HBM), then runs over it
//           front to back: latency by one IEEE add per hop from the source, reliability in the
//           helper's order, the 0 -> 1 latency override, replay-CSR slots replaced by edge ids;
//   place + scatter  routes that fit below the caller's cap get their offset and are copied from
//           staging to the output arrays (one wavefront per route).
// Every store is a plain vector store into memory the call owns.  The walks are dependent random
// 16-B loads, a few per hop: microseconds next to the replay or the keep launch before them.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "topo_chain.h"

namespace shdtopo {

namespace {

using namespace dev;

constexpr int kTB = 256;

__device__ __forceinline__ int64_t gtid() {
    return (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
}
__device__ __forceinline__ int64_t gstride() { return (int64_t)gridDim.x * blockDim.x; }
unsigned grid_for(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kTB - 1) / kTB, 65536));
}

__global__ void trace_fill_i32_kernel(int32_t* __restrict__ p, int32_t v, int64_t n) {
    for (int64_t i = gtid(); i < n; i += gstride()) p[i] = v;
}

__global__ void trace_edge_id_kernel(int64_t V, int64_t E, int directed,
                                     const int32_t* __restrict__ eu,
                                     const int32_t* __restrict__ ev,
                                     const uint32_t* __restrict__ inv,
                                     const int32_t* __restrict__ perm,
                                     const uint32_t* __restrict__ rowptr,
                                     const uint4* __restrict__ rec, int64_t nadj,
                                     int32_t* __restrict__ eid) {
    for (int64_t e = gtid(); e < E; e += gstride()) {
        const int32_t a = eu[e], b = ev[e];
        if (a == b || a < 0 || b < 0 || a >= V || b >= V) continue;
        int64_t j = find_entry(rowptr, rec, perm, inv[a], b);
        if (j >= 0 && j < nadj) atomicMin(&eid[j], (int32_t)e);
        if (!directed) {
            j = find_entry(rowptr, rec, perm, inv[b], a);
            if (j >= 0 && j < nadj) atomicMin(&eid[j], (int32_t)e);
        }
    }
}

// PASS 1: count; PASS 2: write.  One thread per request of the chunk.  PAIR: the chains are the
// batch slots' pair records (topo_chain.h); pass 1 then also marks the chunk sources that have a
// broken chain (broken[i] = 1: the host replays them).
template <int PASS, bool PAIR>
__global__ void __launch_bounds__(kTB)
route_trace_kernel(ReplayCSR g, ReplayWs ws, PairChains pc, TraceIds ids, TraceReqs rq,
                   TraceRoute* __restrict__ routes, int64_t* __restrict__ lneed,
                   int64_t* __restrict__ gneed, const int64_t* __restrict__ loff,
                   int32_t* __restrict__ stV, int32_t* __restrict__ stE,
                   uint8_t* __restrict__ broken) {
    const size_t V = (size_t)g.V;
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        const uint32_t slot = rq.rslot[q], src = rq.rsrc[q], t = rq.rdst[q], idx = rq.ridx[q];
        Chain<PAIR> c;
        const int st = c.open(g, ws, pc, rq, slot, src, t);
        if (st == kChainSkip) continue;
        const bool inr = st == kChainOk;
        if (PASS == 1) {
            int64_t h = -1;
            if (inr && t == src) {
                // path [src]: the self loop (the helper's nVertices == 1 branch)
                if (!isnan(g.selfLat[src])) h = 1;
            } else if (inr) {
                bool bad = !c.reached(g, t);
                uint32_t v = t;
                h = 0;
                while (!bad && v != src) {
                    uint32_t p = 0, j = 0;
                    if (!c.template up<false>(g, ids, v, p, j)) {
                        bad = true;
                        break;
                    }
                    h++;
                    v = p;
                    if (h > (int64_t)V) bad = true;
                }
                if (bad) {
                    h = -1;
                    if (PAIR) broken[slot] = 1;
                }
            }
            TraceRoute r;
            r.offset = -1;
            r.hops = (int32_t)h;
            r.status = h < 0 ? kTraceBroken : kTraceOk;
            r.latency = -1.0;
            r.reliability = -1.0;
            routes[idx] = r;
            const int64_t need = h < 0 ? 0 : h + 1;
            lneed[q] = need;
            gneed[idx] = need;
        } else {
            const int64_t h = routes[idx].hops;
            if (!inr || routes[idx].status != kTraceOk || h < 1) continue;
            const int64_t base = loff[q];
            double lat, rel;
            if (t == src) {
                const int32_t o = ids.perm[src];
                stV[base] = o;
                stV[base + 1] = o;
                stE[base] = ids.selfEid[src];
                stE[base + 1] = -1;
                lat = 0.0 + g.selfLat[src];
                rel = 1.0;
                rel *= (1.0 - g.vloss[src]);
                rel *= (1.0 - g.selfLoss[src]);
            } else {
                // back to front: vertex k of the route at base + k, the replay-CSR slot of hop k
                // (vertex k -> k + 1) parked in stE[base + k]
                uint32_t v = t;
                stV[base + h] = ids.perm[t];
                stE[base + h] = -1;
                for (int64_t k = h - 1; k >= 0; --k) {
                    uint32_t p = 0, j = 0;
                    if (!c.template up<true>(g, ids, v, p, j)) break;  // (pass 1 validated the chain)
                    v = p;
                    stV[base + k] = ids.perm[v];
                    stE[base + k] = (int32_t)j;
                }
                lat = 0.0;
                rel = 1.0;
                rel *= (1.0 - g.vloss[src]);
                rel *= (1.0 - g.vloss[t]);
                for (int64_t k = 0; k < h; ++k) {  // front to back: the helper's order
                    const uint32_t j = (uint32_t)stE[base + k];
                    if ((int64_t)j >= g.nadj) break;
                    const double2 hp = g.hop[j];
                    lat = __dadd_rn(lat, hp.x);
                    rel *= (1.0 - hp.y);
                    stE[base + k] = ids.eid[j];
                }
                if (lat == 0.0) lat = 1.0;
            }
            routes[idx].latency = lat;
            routes[idx].reliability = rel;
        }
    }
}

__global__ void route_trace_place_kernel(int64_t n, TraceRoute* __restrict__ routes,
                                         const int64_t* __restrict__ goff, int64_t cap) {
    for (int64_t i = gtid(); i < n; i += gstride()) {
        if (routes[i].status != kTraceOk) continue;
        const int64_t o = goff[i], need = (int64_t)routes[i].hops + 1;
        if (o + need <= cap) {
            routes[i].offset = o;
        } else {
            routes[i].offset = -1;
            routes[i].status = kTraceCap;
        }
    }
}

// one wavefront per request of the chunk
__global__ void __launch_bounds__(kTB)
route_trace_scatter_kernel(TraceReqs rq, const TraceRoute* __restrict__ routes,
                           const int64_t* __restrict__ loff, const int32_t* __restrict__ stV,
                           const int32_t* __restrict__ stE, int32_t* __restrict__ outV,
                           int32_t* __restrict__ outE) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = gtid() >> 6, nw = gstride() >> 6;
    for (int64_t q = w0; q < rq.n; q += nw) {
        const TraceRoute r = routes[rq.ridx[q]];
        if (r.status != kTraceOk || r.offset < 0) continue;
        const int64_t base = loff[q], cnt = (int64_t)r.hops + 1;
        for (int64_t k = lane; k < cnt; k += 64) {
            outV[r.offset + k] = stV[base + k];
            outE[r.offset + k] = stE[base + k];
        }
    }
}

}  // namespace

hipError_t launch_trace_edge_ids(int64_t V, int64_t E, int directed, const int32_t* eu,
                                 const int32_t* ev, const uint32_t* inv, const int32_t* perm,
                                 const uint32_t* rowptr, const uint4* rec, int64_t nadj,
                                 int32_t* eid, hipStream_t stream) {
    if (nadj <= 0 || E <= 0) return hipSuccess;
    hipLaunchKernelGGL(trace_fill_i32_kernel, dim3(grid_for(nadj)), dim3(kTB), 0, stream, eid,
                       (int32_t)0x7FFFFFFF, nadj);
    hipLaunchKernelGGL(trace_edge_id_kernel, dim3(grid_for(E)), dim3(kTB), 0, stream, V, E,
                       directed, eu, ev, inv, perm, rowptr, rec, nadj, eid);
    return hipGetLastError();
}

hipError_t launch_route_trace_count(const ReplayCSR& g, const ReplayWs& ws, const TraceReqs& rq,
                                    TraceRoute* routes, int64_t* lneed, int64_t* gneed,
                                    hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    hipLaunchKernelGGL((route_trace_kernel<1, false>), dim3(grid_for(rq.n)), dim3(kTB), 0, stream,
                       g, ws, PairChains{}, TraceIds{}, rq, routes, lneed, gneed, nullptr, nullptr,
                       nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_route_trace_count_pairs(const ReplayCSR& g, const PairChains& pc,
                                          const TraceReqs& rq, TraceRoute* routes, int64_t* lneed,
                                          int64_t* gneed, uint8_t* broken, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!rq.rmap || !broken || !pc.prec || !pc.counters || pc.kf < 1 || pc.kf > pc.K)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((route_trace_kernel<1, true>), dim3(grid_for(rq.n)), dim3(kTB), 0, stream,
                       g, ReplayWs{}, pc, TraceIds{}, rq, routes, lneed, gneed, nullptr, nullptr,
                       nullptr, broken);
    return hipGetLastError();
}

hipError_t launch_route_trace_write(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                                    const TraceReqs& rq, TraceRoute* routes, const int64_t* loff,
                                    int32_t* stV, int32_t* stE, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    hipLaunchKernelGGL((route_trace_kernel<2, false>), dim3(grid_for(rq.n)), dim3(kTB), 0, stream,
                       g, ws, PairChains{}, ids, rq, routes, nullptr, nullptr, loff, stV, stE,
                       nullptr);
    return hipGetLastError();
}

hipError_t launch_route_trace_write_pairs(const ReplayCSR& g, const PairChains& pc,
                                          const TraceIds& ids, const TraceReqs& rq,
                                          TraceRoute* routes, const int64_t* loff, int32_t* stV,
                                          int32_t* stE, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!rq.rmap || !pc.prec || !pc.counters || pc.kf < 1 || pc.kf > pc.K)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((route_trace_kernel<2, true>), dim3(grid_for(rq.n)), dim3(kTB), 0, stream,
                       g, ReplayWs{}, pc, ids, rq, routes, nullptr, nullptr, loff, stV, stE,
                       nullptr);
    return hipGetLastError();
}

hipError_t trace_exclusive_scan(const int64_t* in, int64_t* out, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (n > 0x7FFFFFFF) return hipErrorInvalidValue;
    size_t tb = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n, stream);
    if (e != hipSuccess) return e;
    void* tmp = nullptr;
    e = hipMalloc(&tmp, tb ? tb : 1);
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, out, (int)n, stream);
    const hipError_t s = hipStreamSynchronize(stream);  // tmp must outlive the scan
    (void)hipFree(tmp);
    return e != hipSuccess ? e : s;
}

hipError_t launch_route_trace_place(int64_t n, TraceRoute* routes, const int64_t* goff,
                                    int64_t cap, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(route_trace_place_kernel, dim3(grid_for(n)), dim3(kTB), 0, stream, n,
                       routes, goff, cap);
    return hipGetLastError();
}

hipError_t launch_route_trace_scatter(const TraceReqs& rq, const TraceRoute* routes,
                                      const int64_t* loff, const int32_t* stV, const int32_t* stE,
                                      int32_t* outV, int32_t* outE, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(route_trace_scatter_kernel, dim3(grid_for(rq.n * 64)), dim3(kTB), 0,
                       stream, rq, routes, loff, stV, stE, outV, outE);
    return hipGetLastError();
}

}  // namespace shdtopo
