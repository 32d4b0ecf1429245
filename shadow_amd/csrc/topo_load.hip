// topo_load.hip -- link load for gfx950: the weight a set of flows puts on every edge and vertex.
//
// shdtopo_link_load (include/shd_topology_abi.h) sums, over the requested (source, destination,
// weight) flows, the weight crossing every edge (forward and reverse half) and arriving at every
// vertex of the route shdtopo_trace_routes reports.  As for a trace, the heap replay's trace
// launch (topo_replay.hip) leaves igraph's parent of every popped vertex in the slot's vertex
// records; the kernels here walk those chains.  The validation and the per-request walk also run
// over the batch slots' pair records (their <true> forms, topo_chain.h) for the sources a keep
// launch of the batch kernel serves; the tree accumulation keeps its state in the replay slots'
// vertex-record words, so a call with option "load_walk" = 0 replays every source.
//
// All routes of one source share their first hops: a walk per request with one atomic per hop
// puts a whole wavefront on the addresses next to the source.  Per source the union of the
// requested chains is a tree, and the load of the edge into a tree vertex is the weight of the
// requests in its subtree.  So the weights are summed leaf to root, one add per tree vertex:
//
//   validate  one thread per request walks destination -> source with the guards of
//             route_trace_kernel<1> and records the hop count (broken requests take no further
//             part); the last reader of the records' dist words;
//   reset     the dist words (8 B) of the chunk's slots become the u64 subtree weight `acc`, the
//             heap-position word {bit 31: visited, bits 0..30: pending children}; both cleared;
//   claim     a request adds its weight to acc[dst] and walks up, marking vertices; where it sets
//             a mark it counts itself as a pending child of the parent, where the mark is set it
//             stops.  The request that marked its own destination is the candidate starter;
//   push      (a launch of its own: every claim is complete) weights move leaf to root.  A thread
//             arriving at a vertex decrements its count; the one that takes it to zero reads acc
//             and carries it on -- one add into the edge and the vertex accumulator, one into the
//             parent's acc, a fence, then the arrival at the parent -- and every other thread
//             stops.  A starter counts itself in as a child of its own destination (claim), so
//             "starter of a leaf" and "last child of an interior destination" are one rule and
//             no vertex is carried twice.
//
// The words reused are dead once a trace-instantiation replay has ended and the validation has
// read the destinations' dist words, and the next replay of a slot initialises them itself: its
// init loop writes every record's dist word, and a vertex's heap position is stored when it is
// first pushed and not read before (topo_replay.hip: heap_replay_kernel, RpHeap::put).  The heap
// node block is dead as well but holds only V - (LDS positions) nodes per slot: too small for a
// per-vertex u64.
//
// Option "load_walk" = 1 runs the per-request walk instead (two atomics per hop).  Measured at the
// bench size the two are level -- a tree vertex costs seven atomics and a fence,
// and the routes of one source share only 2.8 hops per tree vertex there -- so the walk is the
// default and the tree sums are option "load_walk" = 0; the tests run both.
// Sums are u64 and wrap: any order of the atomics gives the same result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "topo_chain.h"

namespace shdtopo {

namespace {

using namespace dev;
using u64 = unsigned long long;

constexpr int kTB = 256;
constexpr uint32_t kMark = 0x80000000u;
constexpr int32_t kStarter = -2;  // hops[q] of the request that marked its destination

__device__ __forceinline__ int64_t gtid() {
    return (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
}
__device__ __forceinline__ int64_t gstride() { return (int64_t)gridDim.x * blockDim.x; }
unsigned grid_for(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kTB - 1) / kTB, 65536));
}

__device__ __forceinline__ u64* acc_of(uint4* vr, uint32_t v) {
    return reinterpret_cast<u64*>(vr + v);
}
__device__ __forceinline__ uint32_t* state_of(uint4* vr, uint32_t v) {
    return reinterpret_cast<uint32_t*>(vr + v) + 3;
}
__device__ __forceinline__ bool req_in_range(const ReplayCSR& g, const ReplayWs& ws, uint32_t slot,
                                             uint32_t src, uint32_t t) {
    return slot < (uint32_t)ws.slots && src < (uint32_t)g.V && t < (uint32_t)g.V;
}

// one hop p -> v over replay-CSR entry j: w more on the edge (its half by direction) and at v
__device__ __forceinline__ void charge_hop(const TraceIds& ids, const LoadAcc& a, uint32_t j,
                                           uint32_t p, uint32_t v, u64 w) {
    const int32_t e = ids.eid[j];
    if ((uint32_t)e < (uint64_t)a.E) {
        const bool rev = ids.perm[p] != a.eu[e];
        atomicAdd(&a.eload[rev ? a.E + e : (int64_t)e], w);
    }
    atomicAdd(&a.vload[v], w);
}
__device__ __forceinline__ void charge_self(const TraceIds& ids, const LoadAcc& a, uint32_t src,
                                            u64 w) {
    const int32_t e = ids.selfEid[src];
    if ((uint32_t)e < (uint64_t)a.E) atomicAdd(&a.eload[e], w);
    atomicAdd(&a.vload[src], w);
}

// PAIR: the chains are the batch slots' pair records (topo_chain.h); the validation then marks
// the chunk sources that have a broken chain (broken[i] = 1: the host replays them)
template <bool PAIR>
__global__ void __launch_bounds__(kTB)
load_validate_kernel(ReplayCSR g, ReplayWs ws, PairChains pc, TraceReqs rq,
                     const u64* __restrict__ w, int32_t* __restrict__ hops, u64* __restrict__ cnt,
                     uint8_t* __restrict__ broken) {
    const size_t V = (size_t)g.V;
    u64 nok = 0, nbad = 0, hw = 0;
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        const uint32_t slot = rq.rslot[q], src = rq.rsrc[q], t = rq.rdst[q];
        Chain<PAIR> c;
        const int st = c.open(g, ws, pc, rq, slot, src, t);
        if (st == kChainSkip) continue;
        const bool inr = st == kChainOk;
        int64_t h = -1;
        if (inr && t == src) {
            if (!isnan(g.selfLat[src])) h = 1;  // the self loop
        } else if (inr) {
            bool bad = !c.reached(g, t);
            uint32_t v = t;
            h = 0;
            while (!bad && v != src) {
                uint32_t p = 0, j = 0;
                if (!c.template up<false>(g, TraceIds{}, v, p, j)) {
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
        hops[q] = (int32_t)h;
        if (h < 0) {
            nbad++;
        } else {
            nok++;
            hw += w[q] * (u64)h;
        }
    }
    // every lane reaches this point: one atomic per wavefront and counter
    nok = wave_sum_u64(nok);
    nbad = wave_sum_u64(nbad);
    hw = wave_sum_u64(hw);
    if ((threadIdx.x & 63) == 0) {
        if (nok) atomicAdd(&cnt[LD_ROUTED], nok);
        if (nbad) atomicAdd(&cnt[LD_BROKEN], nbad);
        if (hw) atomicAdd(&cnt[LD_HOPW], hw);
    }
}

template <bool PAIR>
__global__ void __launch_bounds__(kTB)
load_walk_kernel(ReplayCSR g, ReplayWs ws, PairChains pc, TraceIds ids, TraceReqs rq,
                 const u64* __restrict__ w, const int32_t* __restrict__ hops, LoadAcc a) {
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        const uint32_t slot = rq.rslot[q], src = rq.rsrc[q], t = rq.rdst[q];
        Chain<PAIR> c;
        if (c.open(g, ws, pc, rq, slot, src, t) != kChainOk) continue;
        int64_t h = hops[q];
        if (h < 1) continue;
        const u64 wq = w[q];
        if (t == src) {
            charge_self(ids, a, src, wq);
            continue;
        }
        uint32_t v = t;
        while (v != src && h-- > 0) {  // (the validation counted h hops)
            uint32_t p = 0, j = 0;
            if (!c.template up<true>(g, ids, v, p, j)) break;
            charge_hop(ids, a, j, p, v, wq);
            v = p;
        }
    }
}

__global__ void __launch_bounds__(kTB)
load_reset_kernel(uint4* __restrict__ vrec, int64_t n) {
    for (int64_t i = gtid(); i < n; i += gstride()) {
        *reinterpret_cast<u64*>(vrec + i) = 0ull;
        reinterpret_cast<uint32_t*>(vrec + i)[3] = 0u;
    }
}

__global__ void __launch_bounds__(kTB)
load_claim_kernel(ReplayCSR g, ReplayWs ws, TraceIds ids, TraceReqs rq, const u64* __restrict__ w,
                  int32_t* __restrict__ hops, LoadAcc a, u64* __restrict__ cnt) {
    const size_t V = (size_t)g.V;
    u64 marked = 0;
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        int64_t h = hops[q];
        if (h < 1) continue;
        const uint32_t slot = rq.rslot[q], src = rq.rsrc[q], t = rq.rdst[q];
        if (!req_in_range(g, ws, slot, src, t)) continue;
        const u64 wq = w[q];
        if (t == src) {
            charge_self(ids, a, src, wq);
            continue;
        }
        uint4* vr = ws.vrec + (size_t)slot * V;
        atomicAdd(acc_of(vr, t), wq);
        uint32_t v = t;
        while (h-- > 0) {  // (at most the validated chain)
            if (atomicOr(state_of(vr, v), kMark) & kMark) break;  // the rest is claimed
            marked++;
            if (v == t) {  // the starter arrives at its destination like a child
                hops[q] = kStarter;
                atomicAdd(state_of(vr, t), 1u);
            }
            const uint32_t j = vr[v].z;
            if ((int64_t)j >= g.nadj) break;
            const uint32_t p = g.own[j];
            if (p == src || p >= (uint32_t)V) break;
            atomicAdd(state_of(vr, p), 1u);  // v is a pending child of p
            v = p;
        }
    }
    marked = wave_sum_u64(marked);
    if ((threadIdx.x & 63) == 0 && marked) atomicAdd(&cnt[LD_TREE], marked);
}

__global__ void __launch_bounds__(kTB)
load_push_kernel(ReplayCSR g, ReplayWs ws, TraceIds ids, TraceReqs rq,
                 const int32_t* __restrict__ hops, LoadAcc a) {
    const size_t V = (size_t)g.V;
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        if (hops[q] != kStarter) continue;
        const uint32_t slot = rq.rslot[q], src = rq.rsrc[q], t = rq.rdst[q];
        if (!req_in_range(g, ws, slot, src, t) || t == src) continue;
        uint4* vr = ws.vrec + (size_t)slot * V;
        // Whoever takes a vertex's count to zero carries its weight on: the starter at its
        // destination (it counted itself in), then the last child to arrive at each parent.
        uint32_t v = t;
        for (size_t guard = 0; guard <= V; ++guard) {
            const uint32_t left = atomicSub(state_of(vr, v), 1u) & ~kMark;
            if (left != 1u) break;  // a child of v is still on its way
            const u64 carry = atomicAdd(acc_of(vr, v), 0ull);
            const uint32_t j = vr[v].z;
            if ((int64_t)j >= g.nadj) break;
            const uint32_t p = g.own[j];
            if (p >= (uint32_t)V) break;
            charge_hop(ids, a, j, p, v, carry);
            if (p == src) break;
            atomicAdd(acc_of(vr, p), carry);
            __threadfence();  // the add is in memory before the count says so
            v = p;
        }
    }
}

__global__ void load_permute_kernel(int64_t V, const int32_t* __restrict__ perm,
                                    const u64* __restrict__ vload, u64* __restrict__ out) {
    for (int64_t v = gtid(); v < V; v += gstride()) {
        const int32_t o = perm[v];
        if ((uint32_t)o < (uint64_t)V) out[o] = vload[v];
    }
}

}  // namespace

hipError_t launch_load_validate(const ReplayCSR& g, const ReplayWs& ws, const TraceReqs& rq,
                                const unsigned long long* w, int32_t* hops,
                                unsigned long long* cnt, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(load_validate_kernel<false>, dim3(grid_for(rq.n)), dim3(kTB), 0, stream, g,
                       ws, PairChains{}, rq, w, hops, cnt, nullptr);
    return hipGetLastError();
}

hipError_t launch_load_validate_pairs(const ReplayCSR& g, const PairChains& pc, const TraceReqs& rq,
                                      const unsigned long long* w, int32_t* hops,
                                      unsigned long long* cnt, uint8_t* broken,
                                      hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!rq.rmap || !broken || !pc.prec || !pc.counters || pc.kf < 1 || pc.kf > pc.K)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(load_validate_kernel<true>, dim3(grid_for(rq.n)), dim3(kTB), 0, stream, g,
                       ReplayWs{}, pc, rq, w, hops, cnt, broken);
    return hipGetLastError();
}

hipError_t launch_load_walk(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                            const TraceReqs& rq, const unsigned long long* w,
                            const int32_t* hops, const LoadAcc& acc, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(load_walk_kernel<false>, dim3(grid_for(rq.n)), dim3(kTB), 0, stream, g, ws,
                       PairChains{}, ids, rq, w, hops, acc);
    return hipGetLastError();
}

hipError_t launch_load_walk_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                  const TraceReqs& rq, const unsigned long long* w,
                                  const int32_t* hops, const LoadAcc& acc, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!rq.rmap || !pc.prec || !pc.counters || pc.kf < 1 || pc.kf > pc.K)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(load_walk_kernel<true>, dim3(grid_for(rq.n)), dim3(kTB), 0, stream, g,
                       ReplayWs{}, pc, ids, rq, w, hops, acc);
    return hipGetLastError();
}

hipError_t launch_load_reset(const ReplayCSR& g, const ReplayWs& ws, int nslots,
                             hipStream_t stream) {
    if (nslots < 1 || g.V <= 0) return hipSuccess;
    if (nslots > ws.slots) return hipErrorInvalidValue;
    const int64_t n = (int64_t)nslots * g.V;
    hipLaunchKernelGGL(load_reset_kernel, dim3(grid_for(n)), dim3(kTB), 0, stream, ws.vrec, n);
    return hipGetLastError();
}

hipError_t launch_load_claim(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                             const TraceReqs& rq, const unsigned long long* w, int32_t* hops,
                             const LoadAcc& acc, unsigned long long* cnt, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(load_claim_kernel, dim3(grid_for(rq.n)), dim3(kTB), 0, stream, g, ws, ids,
                       rq, w, hops, acc, cnt);
    return hipGetLastError();
}

hipError_t launch_load_push(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                            const TraceReqs& rq, const int32_t* hops, const LoadAcc& acc,
                            hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(load_push_kernel, dim3(grid_for(rq.n)), dim3(kTB), 0, stream, g, ws, ids,
                       rq, hops, acc);
    return hipGetLastError();
}

hipError_t launch_load_permute(int64_t V, const int32_t* perm, const unsigned long long* vload,
                               unsigned long long* out, hipStream_t stream) {
    if (V <= 0) return hipSuccess;
    hipLaunchKernelGGL(load_permute_kernel, dim3(grid_for(V)), dim3(kTB), 0, stream, V, perm, vload,
                       out);
    return hipGetLastError();
}

}  // namespace shdtopo
