// topo_chain.h -- the chain sources of the route walks (topo_trace.hip, topo_load.hip).
//
// A walk follows a request's parent chain from its destination back to its source.  The parents
// come from one of two places:
//   Chain<false>  the heap replay's vertex records (its trace launch, topo_replay.hip): word z of
//                 vrec[slot][v] is the replay-CSR entry of v's parent edge, its row the parent;
//   Chain<true>   the batch kernel's pair records (its keep launch, topo_sssp_batch.hip):
//                 prec[slot][v K + lane] = {parent | amb << 31 | bad << 30, tag, f64 loss}, valid
//                 when the tag is the slot's ep | kPairTagClaim and the bad bit is clear (the
//                 epilogue's guards).  A pair record carries no edge: the replay-CSR entry of the
//                 hop parent -> v is found by a binary search of the parent's row.
// Both answer the same question -- the parent p of v and, when asked, the replay-CSR entry j of
// the hop p -> v -- so the walks, their arithmetic and their outputs are one code.
//
// A chunk may mix the two (TraceReqs::rmap): each walk kernel takes the requests of its own chain
// source and leaves the others alone.
#pragma once

#include "topo_dev_common.h"

namespace shdtopo {
namespace dev {

// a vertex record's dist says reached (RpKey::reached of topo_replay.hip, both key encodings)
__device__ __forceinline__ bool rec_reached(const uint4& x, int intKeys) {
    return intKeys ? x.x != 0xFFFFFFFFu : __hiloint2double((int)x.y, (int)x.x) >= 0.0;
}

// entry of row x (relabelled) whose neighbour has ORIGINAL id y: rows ascend by original
// neighbour id (igraph_incident order), one entry per neighbour (parallel groups merged)
__device__ __forceinline__ int64_t find_entry(const uint32_t* __restrict__ rowptr,
                                              const uint4* __restrict__ rec,
                                              const int32_t* __restrict__ perm, uint32_t x,
                                              int32_t y) {
    uint32_t lo = rowptr[x], hi = rowptr[x + 1];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const int32_t o = perm[rec[mid].x];
        if (o == y) return (int64_t)mid;
        if (o < y) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// what Chain::open says of a request
enum { kChainSkip = 0,  // the other chain source's: nothing is read or written for it
       kChainOk = 1,
       kChainBad = 2 };  // out of range: reported broken

template <bool PAIR>
struct Chain;

template <>
struct Chain<false> {
    const uint4* vr = nullptr;
    __device__ __forceinline__ int open(const ReplayCSR& g, const ReplayWs& ws, const PairChains&,
                                        const TraceReqs& rq, uint32_t i, uint32_t src,
                                        uint32_t t) {
        uint32_t slot = i;
        if (rq.rmap) {
            if (i >= rq.nmap) return kChainBad;
            slot = rq.rmap[i];
            if (slot == kNoReplaySlot) return kChainSkip;
        }
        if (slot >= (uint32_t)ws.slots || src >= (uint32_t)g.V || t >= (uint32_t)g.V)
            return kChainBad;
        vr = ws.vrec + (size_t)slot * (size_t)g.V;
        return kChainOk;
    }
    __device__ __forceinline__ bool reached(const ReplayCSR& g, uint32_t t) const {
        return rec_reached(vr[t], g.intKeys);
    }
    // parent p of v and the replay-CSR entry j of the hop p -> v; false: the chain is broken
    template <bool ENTRY>
    __device__ __forceinline__ bool up(const ReplayCSR& g, const TraceIds&, uint32_t v,
                                       uint32_t& p, uint32_t& j) const {
        j = vr[v].z;
        if ((int64_t)j >= g.nadj) return false;
        p = g.own[j];
        return p < (uint32_t)g.V;
    }
};

template <>
struct Chain<true> {
    const uint4* pr = nullptr;  // the slot's records, lane folded in: pr[v K]
    uint32_t K = 0, ept = 0;
    __device__ __forceinline__ int open(const ReplayCSR& g, const ReplayWs&, const PairChains& pc,
                                        const TraceReqs& rq, uint32_t i, uint32_t src,
                                        uint32_t t) {
        if (!rq.rmap || i >= rq.nmap) return kChainBad;
        if (rq.rmap[i] != kNoReplaySlot) return kChainSkip;
        const uint32_t slot = i / (uint32_t)pc.kf, lane = i % (uint32_t)pc.kf;
        if (slot >= (uint32_t)pc.slots || lane >= (uint32_t)pc.K || src >= (uint32_t)g.V ||
            t >= (uint32_t)g.V)
            return kChainBad;
        K = (uint32_t)pc.K;
        pr = pc.prec + (size_t)slot * (size_t)g.V * K + lane;
        const uint32_t ep = (pc.counters[4 * (size_t)slot] - 1u) % kPairTagMask + 1u;
        ept = ep | kPairTagClaim;
        return kChainOk;
    }
    __device__ __forceinline__ bool reached(const ReplayCSR&, uint32_t) const { return true; }
    template <bool ENTRY>
    __device__ __forceinline__ bool up(const ReplayCSR& g, const TraceIds& ids, uint32_t v,
                                       uint32_t& p, uint32_t& j) const {
        const uint4 r = pr[(size_t)v * K];
        if (r.y != ept || (r.x & 0x40000000u)) return false;
        p = r.x & 0x3FFFFFFFu;
        if (p >= (uint32_t)g.V) return false;
        if (ENTRY) {  // rows ascend by original neighbour id; a directed topology: p's out-row
            const int64_t e = find_entry(g.rowptr, g.rec, ids.perm, p, ids.perm[v]);
            if (e < 0 || e >= g.nadj) return false;
            j = (uint32_t)e;
        }
        return true;
    }
};

}  // namespace dev
}  // namespace shdtopo
