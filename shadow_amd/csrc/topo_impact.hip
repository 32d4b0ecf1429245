// topo_impact.hip -- flow impact for gfx950: what changed for a set of flows between two
// device-resident A x A tables.
//
// shdtopo_flow_impact (include/shd_topology_abi.h) joins n flows (srcCol, dstCol, weight) with the
// {latency, reliability} records and the u16 hops of two topologies with the same attached
// vertices.  The tables stay where they are; per flow the join is four random gathers, the access
// pattern of packet_route_kernel (topo_kernels.hip), whose tile this file uses: 256 threads per
// workgroup, workgroup blk owns the flows [blk 256 U, (blk + 1) 256 U), thread t takes the flows
// base + j 256 + t for j < U.  A (wavefront, j) is then 64 consecutive flows and its __ballot is
// word k / 64 of a bitmap of the changed flows.
//
//   count  columns and weights are loaded coalesced and nontemporal, all 4 U gathers are issued
//          before any is used.  Lane 0 writes the ballot word of each (wavefront, j).  Counts come
//          from ballots; the weighted sums are reduced by wave butterflies, meet in LDS and leave
//          as one u64 atomic per non-zero total and workgroup.  The histogram of the delay rises
//          lives in LDS (2 (nb + 1) u64) and only its non-zero bins are flushed.  The per-column
//          weights are global u64 atomics of the changed flows.  Every sum is an integer sum that
//          wraps: any order gives the same result.  The tile's {largest rise, lowest flow reaching
//          it} is merged by topo_paircmp.h's rule, as in diff_count_kernel; the host takes the
//          last step.
//   scan   trace_exclusive_scan over the tiles' changed counts: each tile's first record;
//   fill   the same tiling.  Every thread reads its tile's 4 U words: a changed lane's rank is the
//          tile's offset + the popcounts of the earlier words (flow order: j-major, then
//          wavefront) + the popcount below the lane -- no atomic, no sort, no barrier.  A word
//          that is zero, or starts at or past cap, gathers nothing; only changed lanes gather
//          again and write their 48-B record (three 16-B stores).
//
// No kernel stores outside words [tiles x 4 U], tileChanged / tileRise / tileFlow [tiles], tot
// [IT_COUNT], hist [2 (nb + 1)], srcW / dstW [A], gathered [kImpactShards x kImpactShardStride] and
// out [min(total, cap)]: every index is bounded by k < n (a word's bits are set for flows below n
// only), col < A, bin <= nb or pos < cap.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "topo_dev_common.h"
#include "topo_paircmp.h"

namespace shdtopo {

namespace {

using namespace dev;
using u64 = unsigned long long;

#ifndef SHD_IMPACT_U
#define SHD_IMPACT_U 2
#endif
constexpr int kTB = 256;
constexpr int kNW = kTB / 64;
constexpr int kU = SHD_IMPACT_U;  // flows per thread: 4 kU gathers in flight
constexpr int kWords = kNW * kU;  // ballot words per tile

static_assert(sizeof(ImpactRec) == 48, "ImpactRec is three 16-B stores");
static_assert(kU >= 1 && kU <= 8, "flows per thread");

// LDS of the count pass (all dynamic, u64 words): the totals, the waves' {rise, flow}, the histogram
constexpr int kLdsTot = 0, kLdsRise = IT_COUNT, kLdsFlow = kLdsRise + kNW, kLdsHist = kLdsFlow + kNW;

// the packet route's delay (topo_kernels.hip).  lat is finite and >= 0: attached pairs are connected
// (an infinite or NaN latency would make the cast undefined here as there)
__device__ __forceinline__ u64 delay_ns(double lat) { return (u64)ceil(lat * 1000000.0); }

// the pair index of flow k (-1: an end is no column), its columns to sc / dc
__device__ __forceinline__ int64_t flow_pair(const ImpactFlows& f, int64_t A, int64_t k,
                                             uint32_t* sc, uint32_t* dc) {
    const uint32_t a = (uint32_t)__builtin_nontemporal_load(f.src + k);
    const uint32_t b = (uint32_t)__builtin_nontemporal_load(f.dst + k);
    *sc = a;
    *dc = b;
    return (int64_t)a < A && (int64_t)b < A ? (int64_t)a * A + b : -1;
}

template <class W>
__global__ __launch_bounds__(kTB) void impact_count_kernel(DiffTables t, ImpactFlows f,
                                                           const W* __restrict__ w, ImpactOut o) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const int64_t A = t.A;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int nh = 2 * (f.nb + 1);
    for (int i = (int)threadIdx.x; i < kLdsHist + nh; i += kTB) lds[i] = 0ull;
    __syncthreads();

    const int64_t base = (int64_t)blockIdx.x * (kTB * kU) + threadIdx.x;
    int64_t idx[kU];
    uint32_t sc[kU], dc[kU];
    u64 wt[kU];
#pragma unroll
    for (int j = 0; j < kU; j++) {
        const int64_t k = base + (int64_t)j * kTB;
        idx[j] = -1;
        sc[j] = dc[j] = 0u;
        wt[j] = 0ull;
        if (k < f.n) {
            idx[j] = flow_pair(f, A, k, &sc[j], &dc[j]);
            wt[j] = w ? (u64)__builtin_nontemporal_load(w + k) : 1ull;
        }
    }
    // all 4 kU gathers before any is used: unconditional loads (a flow that is not compared reads
    // pair 0, A > 0, and ignores it), so no branch separates them
    double2 x0[kU], x1[kU];
    uint32_t h0[kU], h1[kU];
#pragma unroll
    for (int j = 0; j < kU; j++) {
        const int64_t x = idx[j] >= 0 ? idx[j] : 0;
        x0[j] = t.lr0[x];
        x1[j] = t.lr1[x];
        h0[j] = t.hops0[x];
        h1[j] = t.hops1[x];
    }

    // wave-uniform counts (from ballots) and per-lane weighted sums
    uint32_t nCompared = 0, nUnattached = 0, nChanged = 0, kc[4] = {0, 0, 0, 0};
    u64 wsum = 0, chw = 0, kw[4] = {0, 0, 0, 0}, dRise = 0, dFall = 0, hRise = 0, hFall = 0;
    double rise = 0.0;
    int64_t flow = -1;
#pragma unroll
    for (int j = 0; j < kU; j++) {
        const int64_t k = base + (int64_t)j * kTB;
        const bool ok = idx[j] >= 0;
        const uint32_t kind = ok ? pair_kind(x0[j], x1[j], h0[j], h1[j]) : 0u;
        const bool ch = ok && pair_changed(x0[j], x1[j], h0[j], h1[j]);
        const u64 mOk = __ballot(ok), mIn = __ballot(k < f.n), m = __ballot(ch);
        if (lane == 0) o.words[(int64_t)blockIdx.x * kWords + j * kNW + wid] = m;
        nCompared += (uint32_t)__popcll(mOk);
        nUnattached += (uint32_t)__popcll(mIn & ~mOk);
        if (ok) wsum += wt[j];
        if (m == 0ull) continue;  // (the same in every lane of the wavefront)
        nChanged += (uint32_t)__popcll(m);
#pragma unroll
        for (int i = 0; i < 4; i++) kc[i] += (uint32_t)__popcll(__ballot((kind >> i) & 1u));
        if (!ch) continue;
        const u64 wj = wt[j];
        chw += wj;
#pragma unroll
        for (int i = 0; i < 4; i++) kw[i] += (kind >> i) & 1u ? wj : 0ull;
        if (h1[j] > h0[j]) hRise += wj * (u64)(h1[j] - h0[j]);
        if (h1[j] < h0[j]) hFall += wj * (u64)(h0[j] - h1[j]);
        if (kind & (kDiffLatRose | kDiffLatFell)) {
            const u64 d0 = delay_ns(x0[j].x), d1 = delay_ns(x1[j].x);
            if (kind & kDiffLatRose) {
                const u64 up = d1 - d0;
                dRise += wj * up;
                // the bin: the number of edges <= up (edges ascend strictly), so bin <= nb
                int lo = 0, hi = f.nb;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (f.edges[mid] <= up) lo = mid + 1;
                    else hi = mid;
                }
                atomicAdd(&lds[kLdsHist + lo], 1ull);
                if (wj) atomicAdd(&lds[kLdsHist + f.nb + 1 + lo], wj);
                const double r = x1[j].x - x0[j].x;
                if (flow < 0 || r > rise) {  // a thread's flows ascend: the first to reach the maximum stays
                    rise = r;
                    flow = k;
                }
            } else {
                dFall += wj * (d0 - d1);
            }
        }
        // sc / dc < A: the flow is compared
        if (wj && o.srcW) atomicAdd(&o.srcW[sc[j]], wj);
        if (wj && o.dstW) atomicAdd(&o.dstW[dc[j]], wj);
    }

    // the wavefront's sums; those of the changed flows only where it has one
    wsum = wave_sum_u64(wsum);
    if (nChanged) {
        chw = wave_sum_u64(chw);
#pragma unroll
        for (int i = 0; i < 4; i++) kw[i] = wave_sum_u64(kw[i]);
        dRise = wave_sum_u64(dRise);
        dFall = wave_sum_u64(dFall);
        hRise = wave_sum_u64(hRise);
        hFall = wave_sum_u64(hFall);
        if (kc[0]) wave_worst_rise(rise, flow);  // {largest rise, lowest flow}
    }
    if (lane == 0) {
        auto add = [&](int i, u64 v) {
            if (v) atomicAdd(&lds[kLdsTot + i], v);
        };
        add(IT_COMPARED, nCompared);
        add(IT_UNATTACHED, nUnattached);
        add(IT_WEIGHT, wsum);
        if (nChanged) {
            add(IT_CHANGED, nChanged);
            add(IT_CHANGED_WEIGHT, chw);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                add(IT_KIND_COUNT + i, kc[i]);
                add(IT_KIND_WEIGHT + i, kw[i]);
            }
            add(IT_DELAY_RISE, dRise);
            add(IT_DELAY_FALL, dFall);
            add(IT_HOPS_RISE, hRise);
            add(IT_HOPS_FALL, hFall);
        }
        lds[kLdsRise + wid] = d2bits(rise);
        lds[kLdsFlow + wid] = (u64)flow;
    }
    __syncthreads();
    if (threadIdx.x < IT_COUNT && lds[kLdsTot + threadIdx.x])
        atomicAdd(&o.tot[threadIdx.x], lds[kLdsTot + threadIdx.x]);
    if (lds[kLdsTot + IT_KIND_COUNT])  // a latency rose in this tile: its bins
        for (int i = (int)threadIdx.x; i < nh; i += kTB)
            if (lds[kLdsHist + i]) atomicAdd(&o.hist[i], lds[kLdsHist + i]);
    if (threadIdx.x == 0) {
        rise = bits2d(lds[kLdsRise]);
        flow = (int64_t)lds[kLdsFlow];
        for (int q = 1; q < kNW; q++) {
            const double r = bits2d(lds[kLdsRise + q]);
            const int64_t c = (int64_t)lds[kLdsFlow + q];
            if (worse_rise(r, c, rise, flow)) {
                rise = r;
                flow = c;
            }
        }
        o.tileChanged[blockIdx.x] = (int64_t)lds[kLdsTot + IT_CHANGED];
        o.tileRise[blockIdx.x] = flow >= 0 ? rise : 0.0;
        o.tileFlow[blockIdx.x] = flow;
    }
}

__global__ __launch_bounds__(kTB) void impact_fill_kernel(DiffTables t, ImpactFlows f,
                                                          const u64* __restrict__ words,
                                                          const int64_t* __restrict__ tileChanged,
                                                          const int64_t* __restrict__ tileOff,
                                                          ImpactRec* __restrict__ out, int64_t cap,
                                                          u64* gathered) {
    // (both conditions are the same for every thread of the workgroup)
    if (tileChanged[blockIdx.x] == 0) return;
    int64_t run = tileOff[blockIdx.x];
    if (run >= cap) return;
    const int64_t A = t.A;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const u64* bw = words + (int64_t)blockIdx.x * kWords;
    // this wavefront's words and the rank of their first changed flow: words in flow order
    u64 mine[kU];
    int64_t first[kU];
#pragma unroll
    for (int q = 0; q < kWords; q++) {
        const u64 m = bw[q];
        if (q % kNW == wid) {
            mine[q / kNW] = m;
            first[q / kNW] = run;
        }
        run += (int64_t)__popcll(m);
    }
    const int64_t base = (int64_t)blockIdx.x * (kTB * kU) + threadIdx.x;
    uint32_t ng = 0;
#pragma unroll
    for (int j = 0; j < kU; j++) {
        const u64 m = mine[j];
        if (m == 0ull || first[j] >= cap) continue;  // (wave-uniform) nothing to gather for
        ng++;
        if (!((m >> lane) & 1ull)) continue;
        const int64_t p = first[j] + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
        if (p >= cap) continue;
        const int64_t k = base + (int64_t)j * kTB;  // (< n: the bit is set)
        uint32_t sc, dc;
        const int64_t x = flow_pair(f, A, k, &sc, &dc);
        if (x < 0) continue;  // (cannot happen: the count pass compared the flow)
        const double2 x0 = t.lr0[x], x1 = t.lr1[x];
        const uint32_t h0 = t.hops0[x], h1 = t.hops1[x];
        ImpactRec r;
        r.flow = k;
        r.lat0 = x0.x;
        r.lat1 = x1.x;
        r.rel0 = x0.y;
        r.rel1 = x1.y;
        r.hops = (h0 & 0xFFFFu) | (h1 << 16);
        r.kind = pair_kind(x0, x1, h0, h1);
        out[p] = r;
    }
    if (lane == 0 && ng)
        atomicAdd(&gathered[(blockIdx.x % kImpactShards) * kImpactShardStride], (u64)ng);
}

int64_t tiles_of(int64_t n) { return (n + kTB * kU - 1) / (kTB * kU); }

}  // namespace

int64_t impact_tile_flows() { return (int64_t)kTB * kU; }

hipError_t launch_impact_count(const DiffTables& t, const ImpactFlows& f,
                               const unsigned long long* w64, const uint32_t* w32,
                               const ImpactOut& o, hipStream_t stream) {
    if (f.n <= 0) return hipSuccess;
    const int64_t tiles = tiles_of(f.n);
    if (tiles > INT32_MAX || f.nb < 0 || f.nb > kImpactMaxEdges || (f.nb > 0 && !f.edges))
        return hipErrorInvalidValue;
    if (t.A <= 0 || !t.lr0 || !t.lr1 || !t.hops0 || !t.hops1) return hipErrorInvalidValue;
    if (!f.src || !f.dst || !o.words || !o.tileChanged || !o.tileRise || !o.tileFlow || !o.tot ||
        !o.hist)
        return hipErrorInvalidValue;
    const size_t lds = sizeof(u64) * (size_t)(kLdsHist + 2 * (f.nb + 1));
    if (w64)
        hipLaunchKernelGGL(impact_count_kernel<u64>, dim3((unsigned)tiles), dim3(kTB), lds, stream,
                           t, f, w64, o);
    else
        hipLaunchKernelGGL(impact_count_kernel<uint32_t>, dim3((unsigned)tiles), dim3(kTB), lds,
                           stream, t, f, w32, o);
    return hipGetLastError();
}

hipError_t launch_impact_fill(const DiffTables& t, const ImpactFlows& f,
                              const unsigned long long* words, const int64_t* tileChanged,
                              const int64_t* tileOff, ImpactRec* out, int64_t cap,
                              unsigned long long* gathered, hipStream_t stream) {
    if (f.n <= 0 || cap <= 0 || t.A <= 0) return hipSuccess;
    const int64_t tiles = tiles_of(f.n);
    if (tiles > INT32_MAX) return hipErrorInvalidValue;
    if (!t.lr0 || !t.lr1 || !t.hops0 || !t.hops1 || !f.src || !f.dst || !words || !tileChanged ||
        !tileOff || !out || !gathered)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(impact_fill_kernel, dim3((unsigned)tiles), dim3(kTB), 0, stream, t, f, words,
                       tileChanged, tileOff, out, cap, gathered);
    return hipGetLastError();
}

}  // namespace shdtopo
