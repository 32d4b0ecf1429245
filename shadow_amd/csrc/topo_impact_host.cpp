// topo_impact_host.cpp -- flow impact (include/shd_topology_abi.h shdtopo_flow_impact*; kernels in
// topo_impact.hip): the flows of one call joined with the two resident tables on the device.
// Locks, the retry loop, errors and side effects are shdtopo_table_diff's (topo_core.cpp).
#include "topo_host.h"

#include <chrono>
#include <cstddef>
#include <functional>

namespace shdtopo {

namespace {

static_assert(sizeof(ShdFlowChange) == 48 && sizeof(ImpactRec) == sizeof(ShdFlowChange) &&
                  offsetof(ShdFlowChange, hops0) == 40 && offsetof(ShdFlowChange, kind) == 44,
              "ImpactRec is the device image of ShdFlowChange");

using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t) {
    return std::chrono::duration<double, std::milli>(clk::now() - t).count();
}

// one call's flows (host variant: IPs and u64 weights; device variant: columns and a u32 payload)
// and its outputs
struct ImpactCall {
    const uint32_t* srcIP = nullptr;
    const uint32_t* dstIP = nullptr;
    const uint64_t* weight = nullptr;
    const int32_t* d_src = nullptr;
    const int32_t* d_dst = nullptr;
    const uint32_t* d_payload = nullptr;
    bool onDevice = false;
    hipStream_t stream = nullptr;
    int64_t n = 0;
    const uint64_t* edges = nullptr;
    int64_t nb = 0;
    ShdFlowChange* out = nullptr;
    int64_t cap = 0;
    ShdImpactTotals* totals = nullptr;
    uint64_t* riseCount = nullptr;
    uint64_t* riseWeight = nullptr;
    uint64_t* srcW = nullptr;
    uint64_t* dstW = nullptr;
};

bool args_ok(Topology* a, Topology* b, const ImpactCall& c) {
    if (!a || !b || c.n < 0 || c.n > 0x7FFFFFFE || c.cap < 0 || (c.cap > 0 && !c.out)) return false;
    if (c.n > 0 && (c.onDevice ? !c.d_src || !c.d_dst : !c.srcIP || !c.dstIP)) return false;
    if (c.nb < 0 || c.nb > kImpactMaxEdges || (c.nb > 0 && !c.edges)) return false;
    for (int64_t i = 1; i < c.nb; i++)
        if (c.edges[i] <= c.edges[i - 1]) return false;
    return true;
}

void zero_outputs(const ImpactCall& c, int64_t A, ShdImpactTotals* tt) {
    *tt = ShdImpactTotals{};
    tt->flows = c.n;
    tt->worstFlow = -1;
    if (c.riseCount) std::fill(c.riseCount, c.riseCount + c.nb + 1, (uint64_t)0);
    if (c.riseWeight) std::fill(c.riseWeight, c.riseWeight + c.nb + 1, (uint64_t)0);
    if (c.srcW) std::fill(c.srcW, c.srcW + A, (uint64_t)0);
    if (c.dstW) std::fill(c.dstW, c.dstW + A, (uint64_t)0);
}

// the host variant's columns (-1: unattached) through a's map; a's build lock is held
void resolve_columns(Topology* a, const ImpactCall& c, std::vector<int32_t>& sc,
                     std::vector<int32_t>& dc) {
    resolve_requests(a, c.srcIP, c.dstIP, c.n, sc, dc);
    for (int64_t i = 0; i < c.n; i++) {
        sc[(size_t)i] = sc[(size_t)i] >= 0 ? a->colOf[(size_t)sc[(size_t)i]] : -1;
        dc[(size_t)i] = dc[(size_t)i] >= 0 ? a->colOf[(size_t)dc[(size_t)i]] : -1;
    }
}

// a == b, or no column at all: nothing can change.  compared / unattached / weight on the host;
// the device variant's arrays are copied over for that (no table is built or read).
int64_t impact_unchanged(Topology* a, const ImpactCall& c, ShdImpactTotals* tt,
                         ShdImpactStats* is) {
    const int64_t A = a->A, n = c.n;
    std::vector<int32_t> sc, dc;
    std::vector<uint32_t> pay;
    if (c.onDevice && n > 0 && A > 0) {
        int r = dev_init(a);
        if (r) return r;
        hipStream_t st = c.stream ? c.stream : a->stream;
        HIPCHK(hipStreamSynchronize(st));
        sc.resize((size_t)n);
        dc.resize((size_t)n);
        HIPCHK(hipMemcpy(sc.data(), c.d_src, 4 * (size_t)n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dc.data(), c.d_dst, 4 * (size_t)n, hipMemcpyDeviceToHost));
        if (c.d_payload) {
            pay.resize((size_t)n);
            HIPCHK(hipMemcpy(pay.data(), c.d_payload, 4 * (size_t)n, hipMemcpyDeviceToHost));
        }
    } else if (!c.onDevice && n > 0) {
        const auto t0 = clk::now();
        resolve_columns(a, c, sc, dc);
        is->resolve_ms = ms_since(t0);
    }
    for (int64_t i = 0; i < n; i++) {
        const bool ok = !sc.empty() && (uint32_t)sc[(size_t)i] < (uint64_t)A &&
                        (uint32_t)dc[(size_t)i] < (uint64_t)A;
        if (!ok) continue;
        tt->compared++;
        tt->weight += c.onDevice ? (pay.empty() ? 1 : pay[(size_t)i]) : (c.weight ? c.weight[i] : 1);
    }
    tt->unattached = n - tt->compared;
    is->words_skipped = (n + 63) / 64;
    return 0;
}

// the impact of two current tables with equal attached sets; the caller holds both build locks
int64_t impact_locked(Topology* a, Topology* b, const ImpactCall& c, ShdImpactTotals* tt,
                      ShdImpactStats* is) {
    const int64_t A = a->A, n = c.n, nb = c.nb;
    zero_outputs(c, A, tt);
    if (a == b || A == 0 || n == 0) return impact_unchanged(a, c, tt, is);
    if (a->devId != b->devId) return -6;
    int r = dev_init(a);  // this thread's HIP device = the tables'
    if (r) return r;
    hipStream_t st = c.onDevice && c.stream ? c.stream : a->stream;
    // (the tables were written on their topologies' streams)
    if (st != a->stream) HIPCHK(hipStreamSynchronize(a->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    DiffTables t;
    t.lr0 = tab_lr(a);
    t.lr1 = tab_lr(b);
    t.hops0 = tab_hops(a);
    t.hops1 = tab_hops(b);
    t.A = (int32_t)A;

    const int64_t T = impact_tile_flows();
    const int64_t tiles = (n + T - 1) / T, nwords = tiles * (T / 64), nh = 2 * (nb + 1);
    DevBuf<int32_t> d_src, d_dst;
    DevBuf<unsigned long long> d_w, d_edges, d_words, d_tot, d_hist, d_srcW, d_dstW, d_gath;
    DevBuf<int64_t> d_cnt, d_off, d_flow;
    DevBuf<double> d_rise;
    DevBuf<ImpactRec> d_out;
    ImpactFlows f;
    f.n = n;
    f.nb = (int32_t)nb;
    const unsigned long long* w64 = nullptr;
    int64_t wbytes = 0;
    if (c.onDevice) {
        f.src = c.d_src;
        f.dst = c.d_dst;
        wbytes = c.d_payload ? 4 : 0;
    } else {
        const auto t0 = clk::now();
        std::vector<int32_t> sc, dc;
        resolve_columns(a, c, sc, dc);
        is->resolve_ms = ms_since(t0);
        HIPCHK(d_src.ensure((size_t)n));
        HIPCHK(d_dst.ensure((size_t)n));
        // (pageable sources: each copy has left its host array when the call returns)
        HIPCHK(hipMemcpyAsync(d_src.p, sc.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_dst.p, dc.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
        if (c.weight) {
            HIPCHK(d_w.ensure((size_t)n));
            HIPCHK(hipMemcpyAsync(d_w.p, c.weight, 8 * (size_t)n, hipMemcpyHostToDevice, st));
            w64 = d_w.p;
            wbytes = 8;
        }
        HIPCHK(hipStreamSynchronize(st));  // sc / dc go out of scope
        f.src = d_src.p;
        f.dst = d_dst.p;
    }
    if (nb > 0) {
        HIPCHK(d_edges.ensure((size_t)nb));
        HIPCHK(hipMemcpyAsync(d_edges.p, c.edges, 8 * (size_t)nb, hipMemcpyHostToDevice, st));
        f.edges = d_edges.p;
    }
    HIPCHK(d_words.ensure((size_t)nwords));
    HIPCHK(d_cnt.ensure((size_t)tiles + 1));
    HIPCHK(d_off.ensure((size_t)tiles + 1));
    HIPCHK(d_rise.ensure((size_t)tiles));
    HIPCHK(d_flow.ensure((size_t)tiles));
    HIPCHK(d_tot.ensure(IT_COUNT));
    HIPCHK(d_hist.ensure((size_t)nh));
    ImpactOut o;
    o.words = d_words.p;
    o.tileChanged = d_cnt.p;
    o.tileRise = d_rise.p;
    o.tileFlow = d_flow.p;
    o.tot = d_tot.p;
    o.hist = d_hist.p;
    HIPCHK(hipMemsetAsync(d_tot.p, 0, 8 * IT_COUNT, st));
    HIPCHK(hipMemsetAsync(d_hist.p, 0, 8 * (size_t)nh, st));
    HIPCHK(hipMemsetAsync(d_cnt.p + tiles, 0, sizeof(int64_t), st));
    if (c.srcW) {
        HIPCHK(d_srcW.ensure((size_t)A));
        HIPCHK(hipMemsetAsync(d_srcW.p, 0, 8 * (size_t)A, st));
        o.srcW = d_srcW.p;
    }
    if (c.dstW) {
        HIPCHK(d_dstW.ensure((size_t)A));
        HIPCHK(hipMemsetAsync(d_dstW.p, 0, 8 * (size_t)A, st));
        o.dstW = d_dstW.p;
    }
    // two event pairs of the call's own: count + scan, and fill (what the host does in between --
    // reading the total, allocating the records -- is not kernel time)
    struct Events {
        hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev;
    for (hipEvent_t& x : ev.e) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipEventRecord(ev.e[0], st));
    HIPCHK(launch_impact_count(t, f, w64, c.onDevice ? c.d_payload : nullptr, o, st));
    HIPCHK(trace_exclusive_scan(d_cnt.p, d_off.p, tiles + 1, st));  // (synchronises st)
    HIPCHK(hipEventRecord(ev.e[1], st));
    int64_t total = 0, gathered = 0;
    unsigned long long gath[kImpactShards * kImpactShardStride] = {};
    HIPCHK(hipMemcpy(&total, d_off.p + tiles, sizeof(int64_t), hipMemcpyDeviceToHost));
    const int64_t nw = std::min(total, c.cap);
    if (nw > 0) {
        HIPCHK(d_out.ensure((size_t)nw));
        HIPCHK(d_gath.ensure(sizeof gath / 8));
        HIPCHK(hipMemsetAsync(d_gath.p, 0, sizeof gath, st));
        HIPCHK(hipEventRecord(ev.e[2], st));
        HIPCHK(launch_impact_fill(t, f, d_words.p, d_cnt.p, d_off.p, d_out.p, c.cap, d_gath.p, st));
        HIPCHK(hipEventRecord(ev.e[3], st));
    }
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    is->kernel_ms = ms;
    if (nw > 0) {
        HIPCHK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
        is->fill_ms = ms;
        is->kernel_ms += ms;
        HIPCHK(hipMemcpy(gath, d_gath.p, sizeof gath, hipMemcpyDeviceToHost));
        for (unsigned long long x : gath) gathered += (int64_t)x;
    }

    unsigned long long tot[IT_COUNT];
    HIPCHK(hipMemcpy(tot, d_tot.p, sizeof tot, hipMemcpyDeviceToHost));
    tt->compared = (int64_t)tot[IT_COMPARED];
    tt->unattached = (int64_t)tot[IT_UNATTACHED];
    tt->changed = (int64_t)tot[IT_CHANGED];
    tt->weight = tot[IT_WEIGHT];
    tt->changedWeight = tot[IT_CHANGED_WEIGHT];
    for (int i = 0; i < 4; i++) {
        tt->kindCount[i] = tot[IT_KIND_COUNT + i];
        tt->kindWeight[i] = tot[IT_KIND_WEIGHT + i];
    }
    tt->delayRiseNs = tot[IT_DELAY_RISE];
    tt->delayFallNs = tot[IT_DELAY_FALL];
    tt->hopsRise = tot[IT_HOPS_RISE];
    tt->hopsFall = tot[IT_HOPS_FALL];
    if (tot[IT_KIND_COUNT]) {
        // the tiles' {largest rise, lowest flow}: tiles ascend with their flows
        std::vector<double> rise((size_t)tiles);
        std::vector<int64_t> flow((size_t)tiles);
        HIPCHK(hipMemcpy(rise.data(), d_rise.p, 8 * (size_t)tiles, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(flow.data(), d_flow.p, 8 * (size_t)tiles, hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < tiles; k++)
            if (flow[(size_t)k] >= 0 && (tt->worstFlow < 0 || rise[(size_t)k] > tt->worstRise)) {
                tt->worstRise = rise[(size_t)k];
                tt->worstFlow = flow[(size_t)k];
            }
    }
    if (nw > 0) HIPCHK(hipMemcpy(c.out, d_out.p, sizeof(ImpactRec) * (size_t)nw, hipMemcpyDeviceToHost));
    std::vector<uint64_t> hist((size_t)nh);
    if (c.riseCount || c.riseWeight)
        HIPCHK(hipMemcpy(hist.data(), d_hist.p, 8 * (size_t)nh, hipMemcpyDeviceToHost));
    if (c.riseCount) std::copy(hist.begin(), hist.begin() + nb + 1, c.riseCount);
    if (c.riseWeight) std::copy(hist.begin() + nb + 1, hist.end(), c.riseWeight);
    if (c.srcW) HIPCHK(hipMemcpy(c.srcW, d_srcW.p, 8 * (size_t)A, hipMemcpyDeviceToHost));
    if (c.dstW) HIPCHK(hipMemcpy(c.dstW, d_dstW.p, 8 * (size_t)A, hipMemcpyDeviceToHost));
    is->words_skipped = (n + 63) / 64 - gathered;
    is->bytes_model = n * (8 + wbytes) + 36 * tt->compared + 8 * nwords + (8 + 36 + 48) * nw;
    return total;
}

// The loop below is the twin of shdtopo_table_diff's in topo_core.cpp (address-ordered build locks,
// compute_geometry, -4, ensure_table, 4 attempts, -5), restated so that the diff stays as it is: a
// change to either belongs in both.
int64_t flow_impact(Topology* a, Topology* b, const ImpactCall& c) {
    if (!args_ok(a, b, c)) return -1;
    const auto t0 = clk::now();
    ShdImpactTotals scratch;
    ShdImpactTotals* tt = c.totals ? c.totals : &scratch;
    auto finish = [&](ShdImpactStats is, int64_t total) {
        is.flows = c.n;
        is.changed = total < 0 ? 0 : total;
        is.total_ms = ms_since(t0);
        a->impactStats = is;
        return total;
    };
    Topology* lo = std::less<Topology*>()(b, a) ? b : a;
    Topology* hi = lo == a ? b : a;
    for (int attempt = 0; attempt < 4; attempt++) {
        {
            // both build locks, the lower address first
            std::unique_lock<std::mutex> l1(lo->buildMu);
            std::unique_lock<std::mutex> l2;
            if (hi != lo) l2 = std::unique_lock<std::mutex>(hi->buildMu);
            compute_geometry(a);
            if (a != b) compute_geometry(b);
            if (a->attached != b->attached) return -4;
            if (a == b || (table_current(a) && table_current(b))) {
                ShdImpactStats is{};
                const int64_t total = impact_locked(a, b, c, tt, &is);
                return finish(is, total);
            }
        }
        // a missing or stale table is built as by shdtopo_build (it takes the build lock itself)
        int r = ensure_table(a);
        if (!r) r = ensure_table(b);
        if (r) return r;
    }
    CRITICAL("the attached sets keep changing while the flows are compared");
    return -5;
}

}  // namespace

}  // namespace shdtopo

extern "C" {

int64_t shdtopo_flow_impact(Topology* a, Topology* b, const uint32_t* srcIP, const uint32_t* dstIP,
                            const uint64_t* weight, int64_t n, const uint64_t* riseEdgeNs,
                            int64_t nb, ShdFlowChange* out, int64_t cap, ShdImpactTotals* totals,
                            uint64_t* riseCount, uint64_t* riseWeight, uint64_t* srcChangedWeight,
                            uint64_t* dstChangedWeight) {
    ImpactCall c;
    c.srcIP = srcIP;
    c.dstIP = dstIP;
    c.weight = weight;
    c.n = n;
    c.edges = riseEdgeNs;
    c.nb = nb;
    c.out = out;
    c.cap = cap;
    c.totals = totals;
    c.riseCount = riseCount;
    c.riseWeight = riseWeight;
    c.srcW = srcChangedWeight;
    c.dstW = dstChangedWeight;
    return flow_impact(a, b, c);
}

int64_t shdtopo_flow_impact_device(Topology* a, Topology* b, const int32_t* d_srcCol,
                                   const int32_t* d_dstCol, const uint32_t* d_payload, int64_t n,
                                   const uint64_t* riseEdgeNs, int64_t nb, ShdFlowChange* out,
                                   int64_t cap, ShdImpactTotals* totals, uint64_t* riseCount,
                                   uint64_t* riseWeight, uint64_t* srcChangedWeight,
                                   uint64_t* dstChangedWeight, void* stream) {
    ImpactCall c;
    c.onDevice = true;
    c.d_src = d_srcCol;
    c.d_dst = d_dstCol;
    c.d_payload = d_payload;
    c.stream = (hipStream_t)stream;
    c.n = n;
    c.edges = riseEdgeNs;
    c.nb = nb;
    c.out = out;
    c.cap = cap;
    c.totals = totals;
    c.riseCount = riseCount;
    c.riseWeight = riseWeight;
    c.srcW = srcChangedWeight;
    c.dstW = dstChangedWeight;
    return flow_impact(a, b, c);
}

int shdtopo_flow_impact_stats(Topology* a, ShdImpactStats* out) {
    const int r = copy_stats(a, &_Topology::impactStats, out);
    if (!r) out->tile_flows = impact_tile_flows();
    return r;
}

}  // extern "C"
