// topo_monitor.hip -- link monitor for gfx950: running per-bin link traffic fed by packet windows.
//
// A link monitor (include/shd_topology_abi.h, "link monitor") keeps the bins of a link timeline in
// HBM across calls and feeds them from packet windows without walking a route.  For a fixed watch
// set and a fixed attached set, a packet's hits depend on its (source column, destination column)
// pair alone: the rows, and the prefix latencies the timeline adds to the emission time.  So
//
//   prepare  once per watch set and attached set: the hit index -- for every ordered column pair
//            its records {ns(prefix latency), row} in hop order, the edge record of a hop before
//            its vertex record, and A x A + 1 offsets over them.  The sources are taken a block
//            (one chunk) at a time; the chains, the validation, the count walk and the mark walk
//            are the crossings' and the timeline's (launch_load_validate[_pairs],
//            launch_cross_count[_pairs], launch_timeline_mark[_pairs]); the fill pass below is the
//            timeline's time walk with the bin atomic replaced by a store into the pair's records;
//   feed     once per packet: two adjacent offsets, the pair's few 16-B records, and one u64
//            atomicAdd per record into the monitor's bins -- TimelineOut::add's bin test on
//            now + offNs.  The packet arrays are streamed with non-temporal loads; the hit
//            counters are summed per wavefront.
//
// Sums are u64 and wrap: any order of the atomics, any split of the packets into feeds, gives the
// same bins.  No LDS, no scratch; everything but the atomics is a plain vector load or store.
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

__device__ __forceinline__ void rec_store(MonRec* __restrict__ rec, int64_t& pos, int64_t end,
                                          int64_t row, u64 off) {
    if (pos < end) rec[pos++] = MonRec{off, (uint32_t)row, 0u};
}

// The timeline's time walk (topo_timeline.hip) for the requests of one block, request ridx being
// the block's pair ridx: its records go to rec[goff[ridx] .. goff[ridx + 1]), never beyond.
template <bool PAIR, bool EDGES>
__global__ void __launch_bounds__(kTB)
monitor_fill_kernel(ReplayCSR g, ReplayWs ws, PairChains pc, TraceIds ids, TraceReqs rq,
                    const int32_t* __restrict__ hops, CrossWatch cw,
                    const int64_t* __restrict__ loff, uint2* __restrict__ stage,
                    const int64_t* __restrict__ goff, MonRec* __restrict__ rec) {
    for (int64_t q = gtid(); q < rq.n; q += gstride()) {
        const uint32_t slot = rq.rslot[q], src = rq.rsrc[q], t = rq.rdst[q];
        Chain<PAIR> c;
        if (c.open(g, ws, pc, rq, slot, src, t) != kChainOk) continue;
        const int64_t h = hops[q];
        const uint32_t pair = rq.ridx[q];
        int64_t pos = goff[pair];
        const int64_t end = goff[pair + 1];
        if (h < 1 || end <= pos) continue;  // no hit: no records
        if (t == src) {
            // the self loop: entered at the emission time, arrival after its latency
            int32_t k = EDGES ? edge_watch(cw, ids.selfEid[src]) : -1;
            if (k >= 0) rec_store(rec, pos, end, k, 0);
            k = vertex_watch(cw, src);
            if (k >= 0) rec_store(rec, pos, end, (int64_t)cw.ne + k, lat_ns(0.0 + g.selfLat[src]));
            continue;
        }
        const int64_t base = loff[q];
        if (loff[q + 1] - base != h) continue;
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
            const u64 enter = lat_ns(lat);
            lat = __dadd_rn(lat, g.hop[s.x].x);
            if (EDGES) {
                const int32_t e = ids.eid[s.x];
                const int32_t ke = edge_watch(cw, e);
                if (ke >= 0)  // the forward rows first, then the reverse rows (a != eu[e])
                    rec_store(rec, pos, end,
                              ids.perm[a] != cw.eu[e] ? (int64_t)cw.ne + ke : (int64_t)ke, enter);
            }
            const int32_t kv = vertex_watch(cw, s.y);
            if (kv >= 0) rec_store(rec, pos, end, (int64_t)cw.ne + kv, lat_ns(lat));
            a = s.y;
        }
    }
}

// out[i] = in[i] + base: a block's record offsets placed in the index
__global__ void __launch_bounds__(kTB)
monitor_offsets_kernel(const int64_t* __restrict__ in, int64_t* __restrict__ out, int64_t n,
                       int64_t base) {
    for (int64_t i = gtid(); i < n; i += gstride()) out[i] = in[i] + base;
}

// hit counters of one thread, summed per wavefront at the kernel's end
struct FeedCount {
    u64 in = 0, before = 0, after = 0, flows = 0, fed = 0, skipped = 0, bad = 0;
};
// TimelineOut::add (topo_flows.cpp) / bin_add (topo_timeline.hip): weight w of row `row` at time t
__device__ __forceinline__ void bin_add(const TimeBins& tb, int64_t row, u64 t, u64 w,
                                        FeedCount& fc) {
    if ((uint64_t)row >= (uint64_t)tb.rows) return;  // (the index rows are below rows)
    u64* outside = tb.acc + tb.rows * tb.nbins + 2 * row;
    if (t < tb.t0) {
        atomicAdd(&outside[0], w);
        fc.before++;
        return;
    }
    if (tb.nbins > 0) {  // (binNs > 0 then)
        const u64 b = (t - tb.t0) / tb.binNs;
        if (b < (u64)tb.nbins) {
            atomicAdd(&tb.acc[row * tb.nbins + (int64_t)b], w);
            fc.in++;
            return;
        }
    }
    atomicAdd(&outside[1], w);
    fc.after++;
}

// One packet per thread and round.  W: the weight's type (u32 payload of a packet batch, u64 of a
// host feed).  cnt: the cumulative counters, then (at MN_COUNT) those of this feed.
template <class W>
__global__ void __launch_bounds__(kTB)
monitor_feed_kernel(int64_t n, const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                    const W* __restrict__ weight, const u64* __restrict__ now,
                    const uint8_t* __restrict__ delivered, MonIndex ix, TimeBins tb,
                    u64* __restrict__ cnt) {
    FeedCount fc;
    for (int64_t k = gtid(); k < n; k += gstride()) {
        if (delivered && __builtin_nontemporal_load(delivered + k) == 0) {
            fc.skipped++;
            continue;
        }
        const uint32_t s = (uint32_t)__builtin_nontemporal_load(src + k);
        const uint32_t d = (uint32_t)__builtin_nontemporal_load(dst + k);
        if (s >= (uint32_t)ix.A || d >= (uint32_t)ix.A) {  // nothing is read through it
            fc.bad++;
            continue;
        }
        fc.fed++;
        const int64_t* o = ix.off + ((int64_t)s * ix.A + d);  // adjacent words: one line
        int64_t r = o[0];
        const int64_t end = std::min<int64_t>(o[1], ix.nrec);
        if (r < 0 || r >= end) continue;
        const u64 w = weight ? (u64)__builtin_nontemporal_load(weight + k) : 1ull;
        const u64 t = now ? __builtin_nontemporal_load(now + k) : 0ull;
        fc.flows++;
        for (; r < end; ++r) {
            const MonRec m = ix.rec[r];
            bin_add(tb, (int64_t)m.row, t + m.offNs, w, fc);
        }
    }
    // every lane reaches this point: one atomic per wavefront and counter
    const u64 v[MN_COUNT] = {wave_sum_u64(fc.in),    wave_sum_u64(fc.before),
                             wave_sum_u64(fc.after), wave_sum_u64(fc.flows),
                             wave_sum_u64(fc.fed),   wave_sum_u64(fc.skipped),
                             wave_sum_u64(fc.bad)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < MN_COUNT; i++)
            if (v[i]) {
                atomicAdd(&cnt[i], v[i]);
                atomicAdd(&cnt[MN_COUNT + i], v[i]);
            }
    }
}

bool watch_ok(const CrossWatch& cw) {
    return cw.ebits && cw.vbits && cw.ne >= 0 && cw.nv >= 0 &&
           (cw.ne == 0 || (cw.eids && cw.eidx && cw.eu)) && (cw.nv == 0 || (cw.vids && cw.vidx));
}
bool pairs_ok(const PairChains& pc, const TraceReqs& rq) {
    return rq.rmap && pc.prec && pc.counters && pc.kf >= 1 && pc.kf <= pc.K;
}

template <class W>
hipError_t feed(int64_t n, const int32_t* src, const int32_t* dst, const W* weight,
                const unsigned long long* now, const uint8_t* delivered, const MonIndex& ix,
                const TimeBins& tb, unsigned long long* cnt, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!src || !dst || !cnt || !tb.acc || tb.rows <= 0 || tb.nbins < 0 ||
        (tb.nbins > 0 && tb.binNs == 0) || !ix.off || ix.A <= 0 || ix.nrec < 0 ||
        (ix.nrec > 0 && !ix.rec))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((monitor_feed_kernel<W>), dim3(grid_for(n)), dim3(kTB), 0, stream, n, src,
                       dst, weight, now, delivered, ix, tb, cnt);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_monitor_fill(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                               const TraceReqs& rq, const int32_t* hops, const CrossWatch& cw,
                               const int64_t* loff, uint2* stage, const int64_t* goff, MonRec* rec,
                               hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!watch_ok(cw) || !goff || !rec) return hipErrorInvalidValue;
    hipLaunchKernelGGL((monitor_fill_kernel<false, true>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                       stream, g, ws, PairChains{}, ids, rq, hops, cw, loff, stage, goff, rec);
    return hipGetLastError();
}

hipError_t launch_monitor_fill_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                     const TraceReqs& rq, const int32_t* hops,
                                     const CrossWatch& cw, const int64_t* loff, uint2* stage,
                                     const int64_t* goff, MonRec* rec, hipStream_t stream) {
    if (rq.n <= 0) return hipSuccess;
    if (!watch_ok(cw) || !pairs_ok(pc, rq) || !goff || !rec) return hipErrorInvalidValue;
    if (cw.ne > 0)
        hipLaunchKernelGGL((monitor_fill_kernel<true, true>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                           stream, g, ReplayWs{}, pc, ids, rq, hops, cw, loff, stage, goff, rec);
    else
        hipLaunchKernelGGL((monitor_fill_kernel<true, false>), dim3(grid_for(rq.n)), dim3(kTB), 0,
                           stream, g, ReplayWs{}, pc, ids, rq, hops, cw, loff, stage, goff, rec);
    return hipGetLastError();
}

hipError_t launch_monitor_offsets(const int64_t* in, int64_t* out, int64_t n, int64_t base,
                                  hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(monitor_offsets_kernel, dim3(grid_for(n)), dim3(kTB), 0, stream, in, out, n,
                       base);
    return hipGetLastError();
}

hipError_t launch_monitor_feed(int64_t n, const int32_t* src, const int32_t* dst,
                               const uint32_t* payload, const unsigned long long* now,
                               const uint8_t* delivered, const MonIndex& ix, const TimeBins& tb,
                               unsigned long long* cnt, hipStream_t stream) {
    return feed<uint32_t>(n, src, dst, payload, now, delivered, ix, tb, cnt, stream);
}

hipError_t launch_monitor_feed_u64(int64_t n, const int32_t* src, const int32_t* dst,
                                   const unsigned long long* weight, const unsigned long long* now,
                                   const uint8_t* delivered, const MonIndex& ix, const TimeBins& tb,
                                   unsigned long long* cnt, hipStream_t stream) {
    return feed<unsigned long long>(n, src, dst, weight, now, delivered, ix, tb, cnt, stream);
}

}  // namespace shdtopo
