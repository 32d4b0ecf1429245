// topo_whatif.cpp -- the link failure what-if family behind the C ABI of
// include/shd_topology_abi.h: derived topologies (shdtopo_derive_without, shdtopo_edge_origin), the
// table diff (shdtopo_table_diff*; kernels in topo_diff.hip), the flow impact
// (shdtopo_flow_impact*; kernels in topo_impact.hip) and the load shift (shdtopo_load_shift*;
// kernels in topo_shift.hip).  The diff and the impact compare the resident tables of two
// topologies: one driver, with_current_pair, takes their locks and brings the tables up to date
// for both.  The shift needs no table: it takes both locks itself, runs the link load's
// accumulation (topo_flows.cpp) on each side and compares the two results where they are.  The
// route schedule (shdtopo_route_schedule*; kernel in topo_schedule.hip) reads the resident tables
// of up to 16 topologies in one packet route: with_current_set is the pair driver over a set.
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "topo_host.h"

namespace shdtopo {

namespace {

static_assert(sizeof(ShdTableChange) == 48 && sizeof(DiffRec) == sizeof(ShdTableChange) &&
                  offsetof(ShdTableChange, hops0) == 40 && offsetof(ShdTableChange, kind) == 44,
              "DiffRec is the device image of ShdTableChange");

static_assert(sizeof(ShdFlowChange) == 48 && sizeof(ImpactRec) == sizeof(ShdFlowChange) &&
                  offsetof(ShdFlowChange, hops0) == 40 && offsetof(ShdFlowChange, kind) == 44,
              "ImpactRec is the device image of ShdFlowChange");

// The pair driver of the diff and the impact: runs locked() under the build locks of a and b (the
// lower address first) once both tables stand for equal attached sets, and returns what it
// returns.  -4: the attached sets differ.  A missing or stale table is built outside the locks and
// the attempt repeated; after four attempts -5 (the sets keep changing while the `what` are
// compared).  sameNeedsTable is the one difference between the callers when a == b: the diff still
// demands a current table and builds one (test_whatif.py test_diff_with_itself_builds_the_table),
// the impact counts on the host and runs locked() without one (test_flow_impact.py
// test_same_topology_builds_no_table).
template <class F>
int64_t with_current_pair(Topology* a, Topology* b, bool sameNeedsTable, const char* what,
                          F&& locked) {
    Topology* lo = std::less<Topology*>()(b, a) ? b : a;
    Topology* hi = lo == a ? b : a;
    for (int attempt = 0; attempt < 4; attempt++) {
        {
            std::unique_lock<std::mutex> l1(lo->buildMu);
            std::unique_lock<std::mutex> l2;
            if (hi != lo) l2 = std::unique_lock<std::mutex>(hi->buildMu);
            compute_geometry(a);
            if (a != b) compute_geometry(b);
            if (a->attached != b->attached) return -4;
            if ((a == b && !sameNeedsTable) || (table_current(a) && table_current(b)))
                return locked();
        }
        // a missing or stale table is built as by shdtopo_build (it takes the build lock itself)
        int r = ensure_table(a);
        if (!r && a != b) r = ensure_table(b);
        if (r) return r;
    }
    CRITICAL("the attached sets keep changing while the %s are compared", what);
    return -5;
}

// The same driver over a set of topologies (the route schedule): mem holds distinct topologies in
// ascending address order, which is the order their build locks are taken in.  locked() runs once
// every member's attached set equals mem[0]'s (else -4) and, when needTables, every table stands;
// stale tables are built outside the locks and the attempt repeated, -5 after four.
template <class F>
int64_t with_current_set(const std::vector<Topology*>& mem, bool needTables, const char* what,
                         F&& locked) {
    for (int attempt = 0; attempt < 4; attempt++) {
        {
            std::vector<std::unique_lock<std::mutex>> locks;
            locks.reserve(mem.size());
            for (Topology* m : mem) locks.emplace_back(m->buildMu);
            for (Topology* m : mem) compute_geometry(m);
            bool current = true;
            for (Topology* m : mem) {
                if (m->attached != mem[0]->attached) return -4;
                current = current && table_current(m);
            }
            if (!needTables || current) return locked();
        }
        for (Topology* m : mem) CHK(ensure_table(m));
    }
    CRITICAL("the attached sets keep changing while the %s are read", what);
    return -5;
}

// the diff of two current tables with equal attached sets; the caller holds both build locks
int64_t diff_locked(Topology* a, Topology* b, ShdTableChange* out, int64_t cap,
                    uint64_t* kindCount, uint32_t* rowChanged, double* rowWorstRise,
                    int32_t* rowWorstCol, ShdDiffStats* ds) {
    const int64_t A = a->A;
    ds->pairs = A * A;
    if (kindCount) std::fill(kindCount, kindCount + 4, (uint64_t)0);
    if (rowChanged) std::fill(rowChanged, rowChanged + (size_t)A, 0u);
    if (rowWorstRise) std::fill(rowWorstRise, rowWorstRise + (size_t)A, 0.0);
    if (rowWorstCol) std::fill(rowWorstCol, rowWorstCol + (size_t)A, (int32_t)-1);
    if (a == b || A == 0) return 0;
    if (a->devId != b->devId) return -6;
    int r = dev_init(a);  // this thread's HIP device = the tables'
    if (r) return r;
    hipStream_t st = a->stream;
    HIPCHK(hipStreamSynchronize(b->stream));  // (b's table was written on b's stream)
    DiffTables t;
    t.lr0 = tab_lr(a);
    t.lr1 = tab_lr(b);
    t.hops0 = tab_hops(a);
    t.hops1 = tab_hops(b);
    t.A = (int32_t)A;
    DevBuf<int64_t> d_cnt, d_off;
    DevBuf<double> d_rise;
    DevBuf<int32_t> d_col;
    DevBuf<unsigned long long> d_kc;
    DevBuf<DiffRec> d_out;
    HIPCHK(d_cnt.ensure((size_t)A + 1));
    HIPCHK(d_off.ensure((size_t)A + 1));
    HIPCHK(d_rise.ensure((size_t)A));
    HIPCHK(d_col.ensure((size_t)A));
    HIPCHK(d_kc.ensure(4));
    DevEvents<2> ev;
    CHK(ev.create());
    HIPCHK(hipMemsetAsync(d_kc.p, 0, 4 * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(d_cnt.p + A, 0, sizeof(int64_t), st));
    HIPCHK(hipEventRecord(ev.e[0], st));
    HIPCHK(launch_diff_count(t, d_cnt.p, d_rise.p, d_col.p, d_kc.p, st));
    HIPCHK(trace_exclusive_scan(d_cnt.p, d_off.p, A + 1, st));  // (synchronises st)
    std::vector<int64_t> cnt((size_t)A), off((size_t)A + 1);
    HIPCHK(hipMemcpy(cnt.data(), d_cnt.p, sizeof(int64_t) * (size_t)A, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(off.data(), d_off.p, sizeof(int64_t) * ((size_t)A + 1), hipMemcpyDeviceToHost));
    const int64_t total = off[(size_t)A];
    const int64_t nw = std::min(total, cap);
    int64_t filled = 0;  // rows the fill pass walks
    if (nw > 0) {
        HIPCHK(d_out.ensure((size_t)nw));
        HIPCHK(launch_diff_fill(t, d_cnt.p, d_off.p, d_out.p, cap, st));
        for (int64_t s = 0; s < A; s++) filled += cnt[(size_t)s] > 0 && off[(size_t)s] < cap ? 1 : 0;
    }
    HIPCHK(hipEventRecord(ev.e[1], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    ds->kernel_ms = ms;
    ds->bytes_read = 36 * (A * A + filled * A);
    if (nw > 0) HIPCHK(hipMemcpy(out, d_out.p, sizeof(DiffRec) * (size_t)nw, hipMemcpyDeviceToHost));
    if (kindCount) HIPCHK(hipMemcpy(kindCount, d_kc.p, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (rowChanged)
        for (int64_t s = 0; s < A; s++) rowChanged[s] = (uint32_t)cnt[(size_t)s];
    if (rowWorstRise)
        HIPCHK(hipMemcpy(rowWorstRise, d_rise.p, sizeof(double) * (size_t)A, hipMemcpyDeviceToHost));
    if (rowWorstCol)
        HIPCHK(hipMemcpy(rowWorstCol, d_col.p, sizeof(int32_t) * (size_t)A, hipMemcpyDeviceToHost));
    return total;
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
        const auto t0 = std::chrono::steady_clock::now();
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
        const auto t0 = std::chrono::steady_clock::now();
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
    DevEvents<4> ev;
    CHK(ev.create());
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

int64_t flow_impact(Topology* a, Topology* b, const ImpactCall& c) {
    if (!args_ok(a, b, c)) return -1;
    const auto t0 = std::chrono::steady_clock::now();
    ShdImpactTotals scratch;
    ShdImpactTotals* tt = c.totals ? c.totals : &scratch;
    auto finish = [&](ShdImpactStats is, int64_t total) {
        is.flows = c.n;
        is.changed = total < 0 ? 0 : total;
        is.total_ms = ms_since(t0);
        a->impactStats = is;
        return total;
    };
    return with_current_pair(a, b, false, "flows", [&] {
        ShdImpactStats is{};
        const int64_t total = impact_locked(a, b, c, tt, &is);
        return finish(is, total);
    });
}

// ---- load shift (shdtopo_load_shift; kernels in topo_shift.hip) ----

static_assert(sizeof(ShdLoadChange) == 32 && sizeof(ShiftRec) == sizeof(ShdLoadChange) &&
                  offsetof(ShdLoadChange, idA) == offsetof(ShiftRec, idA) &&
                  offsetof(ShdLoadChange, before) == 16 && offsetof(ShiftRec, before) == 16,
              "ShiftRec is the device image of ShdLoadChange");

int64_t root_edges(const Topology* t) { return t->rootE >= 0 ? t->rootE : t->g.E; }

// The root edge ids t lacks, ascending: the complement of its origins in [0, R).  false: the
// origins are not E strictly ascending ids of [0, R) (so the gaps are R - E distinct ids, which is
// what bounds the kernels' loads).
bool root_gaps(const Topology* t, int64_t R, std::vector<int32_t>& gaps) {
    gaps.clear();
    const int64_t E = t->g.E;
    if (t->edgeOrigin.empty()) return E == R;
    if ((int64_t)t->edgeOrigin.size() != E || E > R) return false;
    int64_t next = 0;
    for (int64_t e = 0; e < E; e++) {
        const int64_t r = t->edgeOrigin[(size_t)e];
        if (r < next || r >= R) return false;
        for (; next < r; next++) gaps.push_back((int32_t)next);
        next = r + 1;
    }
    for (; next < R; next++) gaps.push_back((int32_t)next);
    return true;
}

// one side of a shift: the load of the call's flows on one topology
struct ShiftLoad {
    Topology* top = nullptr;
    std::vector<int32_t> gaps;
    bool onHost = false;               // a complete topology: accumulated on the host
    std::vector<uint64_t> eload, vload;  // ... into these (u64 [2 E], u64 [V])
    LoadSums dev;                      // the sums on the device (a host side's upload)
    ShdLoadStats ls{};
    double ms = 0.0;
    // the host image of kernel's side_id: the side's id of root edge r, -1: it lacks it
    int32_t id_of(int32_t r) const {
        const auto it = std::lower_bound(gaps.begin(), gaps.end(), r);
        if (it != gaps.end() && *it == r) return -1;
        return r - (int32_t)(it - gaps.begin());
    }
};

// the accumulation of one side as shdtopo_link_load runs it, its statistics into s.ls
int shift_accumulate(ShiftLoad& s, const std::vector<int32_t>& sv, const std::vector<int32_t>& dv,
                     const uint64_t* weight, int64_t n, int64_t nvalid) {
    const auto t0 = std::chrono::steady_clock::now();
    Topology* top = s.top;
    ChainStats cs;
    s.ls = ShdLoadStats{};
    s.ls.requests = n;
    s.ls.unattached = n - nvalid;
    int r = 0;
    if (top->isComplete) {
        s.onHost = true;
        s.eload.assign(2 * (size_t)top->g.E, 0);
        s.vload.assign((size_t)top->g.V, 0);
        load_complete(top, sv, dv, weight, n, s.eload.data(), s.vload.data(), &s.ls);
    } else {
        r = load_accumulate(top, sv, dv, weight, n, s.dev, &s.ls, cs);
    }
    cs.out(&s.ls, &ShdLoadStats::load_kernel_ms);
    s.ls.ids_ms = cs.ids_ms;
    s.ls.total_ms = s.ms = ms_since(t0);
    return r;
}

// a host side's sums to the device (the other side is not complete); the device is bound
int shift_upload(ShiftLoad& s) {
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(s.dev.d_eload.ensure(s.eload.size()));
    HIPCHK(s.dev.d_vout.ensure(s.vload.size()));
    if (!s.eload.empty())
        HIPCHK(hipMemcpy(s.dev.d_eload.p, s.eload.data(), 8 * s.eload.size(), hipMemcpyHostToDevice));
    if (!s.vload.empty())
        HIPCHK(hipMemcpy(s.dev.d_vout.p, s.vload.data(), 8 * s.vload.size(), hipMemcpyHostToDevice));
    s.ms += ms_since(t0);
    s.ls.total_ms = s.ms;
    return 0;
}

// what one changed or unchanged entry adds to the totals (the host image of shift_count_kernel)
struct ShiftFold {
    ShdShiftTotals* tt;
    void peak(int64_t x, uint64_t before, uint64_t after) const {
        if (before > tt->peakBefore) {  // ascending x: the first to reach the maximum stays
            tt->peakBefore = before;
            tt->peakBeforeIndex = x;
        }
        if (after > tt->peakAfter) {
            tt->peakAfter = after;
            tt->peakAfterIndex = x;
        }
    }
    void change(int64_t x, const ShdLoadChange& c) const {
        const int k = c.kind;
        tt->changed[k]++;
        if (c.after > c.before) {
            const uint64_t d = c.after - c.before;
            tt->gained[k]++;
            tt->gainedWeight[k] += d;
            if (c.before == 0) tt->newlyUsed[k]++;
            if (d > tt->worstGain) {
                tt->worstGain = d;
                tt->worstGainIndex = x;
            }
        } else {
            const uint64_t d = c.before - c.after;
            tt->lost[k]++;
            tt->lostWeight[k] += d;
            if (c.after == 0) tt->abandoned[k]++;
            if (d > tt->worstLoss) {
                tt->worstLoss = d;
                tt->worstLossIndex = x;
            }
        }
        if (k < 2 && c.idB < 0) tt->displaced += c.before;
        if (k < 2 && c.idA < 0) tt->appeared += c.after;
    }
};

// both sides on the host (two complete topologies): the whole answer without a device
int64_t shift_on_host(const ShiftLoad& sa, const ShiftLoad& sb, int64_t R, int64_t V,
                      ShdLoadChange* out, int64_t cap, ShdShiftTotals* tt) {
    const ShiftFold fold{tt};
    const int64_t Ea = sa.top->g.E, Eb = sb.top->g.E;
    int64_t total = 0;
    for (int64_t x = 0; x < 2 * R + V; x++) {
        ShdLoadChange c;
        if (x >= 2 * R) {
            c.kind = 2;
            c.id = c.idA = c.idB = (int32_t)(x - 2 * R);
            c.before = sa.vload[(size_t)c.id];
            c.after = sb.vload[(size_t)c.id];
        } else {
            c.kind = x >= R ? 1 : 0;
            c.id = (int32_t)(c.kind ? x - R : x);
            c.idA = sa.id_of(c.id);
            c.idB = sb.id_of(c.id);
            c.before = c.idA >= 0 ? sa.eload[(size_t)(c.kind * Ea + c.idA)] : 0;
            c.after = c.idB >= 0 ? sb.eload[(size_t)(c.kind * Eb + c.idB)] : 0;
            fold.peak(x, c.before, c.after);
        }
        if (c.before == c.after) continue;
        fold.change(x, c);
        if (total < cap) out[total] = c;
        total++;
    }
    return total;
}

// both sides on the device: the compare kernels on a's stream, events of the call's own
int64_t shift_on_device(Topology* a, const ShiftLoad& sa, const ShiftLoad& sb, int64_t R, int64_t V,
                        ShdLoadChange* out, int64_t cap, ShdShiftTotals* tt, ShdShiftStats* ss) {
    hipStream_t st = a->stream;
    DevBuf<int32_t> d_gapsA, d_gapsB;
    auto side = [&](const ShiftLoad& s, DevBuf<int32_t>& d_gaps, ShiftSide* o) {
        const size_t ng = s.gaps.size();
        if (ng) {
            HIPCHK(d_gaps.ensure(ng));
            HIPCHK(hipMemcpy(d_gaps.p, s.gaps.data(), 4 * ng, hipMemcpyHostToDevice));
        }
        *o = ShiftSide{s.dev.d_eload.p, s.dev.d_vout.p, ng ? d_gaps.p : nullptr, (int32_t)ng,
                       s.top->g.E};
        return 0;
    };
    ShiftIn in;
    in.R = R;
    in.V = V;
    CHK(side(sa, d_gapsA, &in.a));
    if (&sb == &sa) in.b = in.a;
    else CHK(side(sb, d_gapsB, &in.b));

    const int64_t X = 2 * R + V, T = shift_tile_entries();
    const int64_t tiles = (X + T - 1) / T, nwords = tiles * (T / 64);
    DevBuf<unsigned long long> d_words, d_tval, d_tot, d_pval, d_gath;
    DevBuf<int64_t> d_cnt, d_off, d_tidx, d_pidx;
    DevBuf<ShiftRec> d_out;
    HIPCHK(d_words.ensure((size_t)nwords));
    HIPCHK(d_cnt.ensure((size_t)tiles + 1));
    HIPCHK(d_off.ensure((size_t)tiles + 1));
    HIPCHK(d_tval.ensure((size_t)tiles * SP_COUNT));
    HIPCHK(d_tidx.ensure((size_t)tiles * SP_COUNT));
    HIPCHK(d_tot.ensure(SH_COUNT));
    HIPCHK(d_pval.ensure(SP_COUNT));
    HIPCHK(d_pidx.ensure(SP_COUNT));
    ShiftOut o;
    o.words = d_words.p;
    o.tileChanged = d_cnt.p;
    o.tileVal = d_tval.p;
    o.tileIdx = d_tidx.p;
    o.tot = d_tot.p;
    HIPCHK(hipMemsetAsync(d_tot.p, 0, 8 * SH_COUNT, st));
    HIPCHK(hipMemsetAsync(d_cnt.p + tiles, 0, sizeof(int64_t), st));
    // two event pairs of the call's own: count + reduce + scan, and fill (what the host does in
    // between -- reading the total, allocating the records -- is not kernel time)
    DevEvents<4> ev;
    CHK(ev.create());
    HIPCHK(hipEventRecord(ev.e[0], st));
    HIPCHK(launch_shift_count(in, o, st));
    HIPCHK(launch_shift_reduce(tiles, d_tval.p, d_tidx.p, d_pval.p, d_pidx.p, st));
    HIPCHK(trace_exclusive_scan(d_cnt.p, d_off.p, tiles + 1, st));  // (synchronises st)
    HIPCHK(hipEventRecord(ev.e[1], st));
    int64_t total = 0, gathered = 0;
    unsigned long long gath[kImpactShards * kImpactShardStride] = {};
    HIPCHK(hipMemcpy(&total, d_off.p + tiles, sizeof(int64_t), hipMemcpyDeviceToHost));
    const int64_t nw = std::min(total, cap);
    if (nw > 0) {
        HIPCHK(d_out.ensure((size_t)nw));
        HIPCHK(d_gath.ensure(sizeof gath / 8));
        HIPCHK(hipMemsetAsync(d_gath.p, 0, sizeof gath, st));
        HIPCHK(hipEventRecord(ev.e[2], st));
        HIPCHK(launch_shift_fill(in, d_words.p, d_cnt.p, d_off.p, d_out.p, cap, d_gath.p, st));
        HIPCHK(hipEventRecord(ev.e[3], st));
    }
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    ss->kernel_ms = ms;
    if (nw > 0) {
        HIPCHK(hipEventElapsedTime(&ms, ev.e[2], ev.e[3]));
        ss->kernel_ms += ms;
        HIPCHK(hipMemcpy(gath, d_gath.p, sizeof gath, hipMemcpyDeviceToHost));
        for (unsigned long long x : gath) gathered += (int64_t)x;
        HIPCHK(hipMemcpy(out, d_out.p, sizeof(ShiftRec) * (size_t)nw, hipMemcpyDeviceToHost));
    }
    unsigned long long tot[SH_COUNT], pval[SP_COUNT];
    int64_t pidx[SP_COUNT];
    HIPCHK(hipMemcpy(tot, d_tot.p, sizeof tot, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pval, d_pval.p, sizeof pval, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pidx, d_pidx.p, sizeof pidx, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) {
        tt->changed[k] = (int64_t)tot[SH_CHANGED + k];
        tt->gained[k] = (int64_t)tot[SH_GAINED + k];
        tt->lost[k] = (int64_t)tot[SH_LOST + k];
        tt->newlyUsed[k] = (int64_t)tot[SH_NEW + k];
        tt->abandoned[k] = (int64_t)tot[SH_ABANDONED + k];
        tt->gainedWeight[k] = tot[SH_GAINED_W + k];
        tt->lostWeight[k] = tot[SH_LOST_W + k];
    }
    tt->displaced = tot[SH_DISPLACED];
    tt->appeared = tot[SH_APPEARED];
    tt->worstGain = pval[SP_GAIN];
    tt->worstGainIndex = pidx[SP_GAIN];
    tt->worstLoss = pval[SP_LOSS];
    tt->worstLossIndex = pidx[SP_LOSS];
    tt->peakBefore = pval[SP_PEAK_BEFORE];
    tt->peakBeforeIndex = pidx[SP_PEAK_BEFORE];
    tt->peakAfter = pval[SP_PEAK_AFTER];
    tt->peakAfterIndex = pidx[SP_PEAK_AFTER];
    ss->words_skipped = (X + 63) / 64 - gathered;
    ss->bytes_model = 8 * (2 * in.a.E + V) + 8 * (2 * in.b.E + V) + 8 * nwords +
                      (8 + 16 * SP_COUNT) * tiles + (16 + 32) * nw;
    return total;
}

// the shift under both build locks; a's statistics are the caller's to store
int64_t shift_locked(Topology* a, Topology* b, const uint32_t* srcIP, const uint32_t* dstIP,
                     const uint64_t* weight, int64_t n, ShdLoadChange* out, int64_t cap,
                     ShdShiftTotals* tt, ShdShiftStats* ss) {
    const int64_t R = root_edges(a), V = a->g.V;
    *tt = ShdShiftTotals{};
    tt->flows = n;
    tt->worstGainIndex = tt->worstLossIndex = tt->peakBeforeIndex = tt->peakAfterIndex = -1;
    ss->entries = 2 * R + V;
    ss->words_skipped = (ss->entries + 63) / 64;
    ShiftLoad la, lb;
    la.top = a;
    lb.top = b;
    if (!root_gaps(a, R, la.gaps) || (a != b && !root_gaps(b, R, lb.gaps))) return -7;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> sv, dv;
    const int64_t nvalid = resolve_requests(a, srcIP, dstIP, n, sv, dv);
    ss->resolve_ms = ms_since(t0);
    tt->unattached = n - nvalid;
    ShiftLoad& rb = a == b ? la : lb;
    const bool host = a->isComplete && b->isComplete;
    if (nvalid == 0) {  // nothing is routed on either side: every load is 0, no device is used
        la.ls.requests = n;
        la.ls.unattached = n;
        ss->loadA = ss->loadB = la.ls;
        return 0;
    }
    if (!host) {  // this thread's HIP device = both sides'
        int r = dev_init(a);
        if (!r && a != b) r = dev_init(b);
        if (r) return r;
        if (a->devId != b->devId) return -6;
    }
    int r = shift_accumulate(la, sv, dv, weight, n, nvalid);
    if (!r && !host && la.onHost) r = shift_upload(la);
    ss->load_a_ms = la.ms;
    ss->loadA = ss->loadB = la.ls;
    if (!r && a != b) {
        r = shift_accumulate(lb, sv, dv, weight, n, nvalid);
        if (!r && !host && lb.onHost) r = shift_upload(lb);
        ss->load_b_ms = lb.ms;
        ss->loadB = lb.ls;
    }
    if (r) return r;
    tt->routedA = la.ls.routed;
    tt->brokenA = la.ls.broken;
    tt->hopWeightA = la.ls.hop_weight;
    tt->routedB = rb.ls.routed;
    tt->brokenB = rb.ls.broken;
    tt->hopWeightB = rb.ls.hop_weight;
    if (host) return shift_on_host(la, rb, R, V, out, cap, tt);
    r = dev_init(a);  // (b's accumulation bound b's stream's device: the same one)
    if (r) return r;
    return shift_on_device(a, la, rb, R, V, out, cap, tt, ss);
}

int64_t load_shift(Topology* a, Topology* b, const uint32_t* srcIP, const uint32_t* dstIP,
                   const uint64_t* weight, int64_t n, ShdLoadChange* out, int64_t cap,
                   ShdShiftTotals* totals) {
    if (!a || !b || n < 0 || n > 0x7FFFFFFE || cap < 0 || (cap > 0 && !out)) return -1;
    if (n > 0 && (!srcIP || !dstIP)) return -1;
    const auto t0 = std::chrono::steady_clock::now();
    Topology* lo = std::less<Topology*>()(b, a) ? b : a;
    Topology* hi = lo == a ? b : a;
    std::unique_lock<std::mutex> l1(lo->buildMu);
    std::unique_lock<std::mutex> l2;
    if (hi != lo) l2 = std::unique_lock<std::mutex>(hi->buildMu);
    if (a->g.V != b->g.V || root_edges(a) != root_edges(b)) return -7;
    compute_geometry(a);
    if (a != b) compute_geometry(b);
    if (a->attached != b->attached) return -4;
    ShdShiftTotals scratch;
    ShdShiftStats ss{};
    const int64_t total = shift_locked(a, b, srcIP, dstIP, weight, n, out, cap,
                                       totals ? totals : &scratch, &ss);
    ss.changed = total < 0 ? 0 : total;
    ss.total_ms = ms_since(t0);
    a->shiftStats = ss;
    return total;
}

// ---- route schedule (shdtopo_route_schedule*; kernel in topo_schedule.hip) ----

static_assert(SHD_SCHEDULE_MAX == kScheduleMax, "the ABI's limit is the kernel argument's");

// one call: the schedule, the window (device variant: device arrays; host variant: vertices, -1 =
// the address is not attached) and its outputs
struct ScheduleCall {
    Topology* const* tops = nullptr;
    const uint64_t* fromNs = nullptr;
    int k = 0;
    bool onDevice = false;
    const int32_t* src = nullptr;  // columns on the device / vertices on the host
    const int32_t* dst = nullptr;
    const uint32_t* payload = nullptr;
    const uint32_t* stateIn = nullptr;
    const uint64_t* now = nullptr;
    int64_t n = 0;
    uint64_t jumpNs = 0;
    int clamp = 0;
    uint64_t* d_time = nullptr;  // device variant
    uint32_t* d_stateOut = nullptr;
    uint8_t* d_delivered = nullptr;
    TopoPacketOut* out = nullptr;  // host variant
    uint8_t* epoch = nullptr;      // device / host array, may be NULL
    uint64_t* epochCount = nullptr;
    hipStream_t stream = nullptr;
};

bool schedule_ok(Topology* const* tops, const uint64_t* fromNs, int k) {
    if (!tops || !fromNs || k < 1 || k > SHD_SCHEDULE_MAX || fromNs[0] != 0) return false;
    for (int e = 0; e < k; e++)
        if (!tops[e] || (e > 0 && fromNs[e] <= fromNs[e - 1])) return false;
    return true;
}

bool args_ok(const ScheduleCall& c) {
    if (!schedule_ok(c.tops, c.fromNs, c.k) || c.n < 0) return false;
    if (c.n == 0) return true;
    if (!c.src || !c.dst || !c.payload || !c.stateIn || !c.now) return false;
    return c.onDevice ? c.d_time && c.d_stateOut && c.d_delivered : c.out != nullptr;
}

// the distinct members of a schedule in ascending address order
std::vector<Topology*> schedule_members(Topology* const* tops, int k) {
    std::vector<Topology*> mem(tops, tops + k);
    std::sort(mem.begin(), mem.end(), std::less<Topology*>());
    mem.erase(std::unique(mem.begin(), mem.end()), mem.end());
    return mem;
}

// the schedule over current tables with equal attached sets; the caller holds every member's
// build lock.  Returns the packets not routed (the device variant: 0).
int64_t schedule_locked(const ScheduleCall& c, const std::vector<Topology*>& mem,
                        ShdScheduleStats* ss) {
    Topology* t0 = c.tops[0];
    const int64_t A = t0->A;
    const size_t n = (size_t)c.n;
    const int k = c.k;
    if (c.epochCount) std::fill(c.epochCount, c.epochCount + 3 * k, (uint64_t)0);
    if (n == 0) return 0;
    for (Topology* m : mem)
        if (m->devId != t0->devId) return -6;
    CHK(dev_init(t0));  // this thread's HIP device = the tables'
    hipStream_t st = c.onDevice && c.stream ? c.stream : t0->stream;
    // (each member's table was written on its own stream)
    for (Topology* m : mem)
        if (m->stream != st) HIPCHK(hipStreamSynchronize(m->stream));
    ScheduleTables T;
    T.k = k;
    for (int e = 0; e < k; e++) {
        T.lr[e] = tab_lr(c.tops[e]);
        T.from[e] = c.fromNs[e];
    }
    const int32_t *d_src = c.src, *d_dst = c.dst;
    const uint32_t *d_pay = c.payload, *d_sin = c.stateIn;
    const uint64_t* d_now = c.now;
    uint64_t* d_time = c.d_time;
    uint32_t* d_sout = c.d_stateOut;
    uint8_t *d_dl = c.d_delivered, *d_ep = c.epoch;
    std::vector<int32_t> sc, dc;
    int64_t bad = 0;
    if (!c.onDevice) {
        // the vertices' columns through tops[0], by route_vertices' rule; the staging is tops[0]'s
        sc.resize(n);
        dc.resize(n);
        for (size_t i = 0; i < n; i++) {
            sc[i] = c.src[i] >= 0 && c.src[i] < t0->g.V ? t0->colOf[(size_t)c.src[i]] : -1;
            dc[i] = c.dst[i] >= 0 && c.dst[i] < t0->g.V ? t0->colOf[(size_t)c.dst[i]] : -1;
            if (sc[i] < 0 || dc[i] < 0 || sc[i] >= A || dc[i] >= A) {
                sc[i] = dc[i] = -1;  // not routed (the kernel leaves it undelivered)
                bad++;
            }
        }
        HIPCHK(t0->b_src.ensure(n)); HIPCHK(t0->b_dst.ensure(n)); HIPCHK(t0->b_pay.ensure(n));
        HIPCHK(t0->b_sin.ensure(n)); HIPCHK(t0->b_sout.ensure(n)); HIPCHK(t0->b_now.ensure(n));
        HIPCHK(t0->b_time.ensure(n)); HIPCHK(t0->b_dl.ensure(n));
        if (c.epoch) HIPCHK(t0->b_ep.ensure(n));
        HIPCHK(hipMemcpyAsync(t0->b_src.p, sc.data(), 4 * n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(t0->b_dst.p, dc.data(), 4 * n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(t0->b_pay.p, c.payload, 4 * n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(t0->b_sin.p, c.stateIn, 4 * n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(t0->b_now.p, c.now, 8 * n, hipMemcpyHostToDevice, st));
        d_src = t0->b_src.p;
        d_dst = t0->b_dst.p;
        d_pay = t0->b_pay.p;
        d_sin = t0->b_sin.p;
        d_now = t0->b_now.p;
        d_time = t0->b_time.p;
        d_sout = t0->b_sout.p;
        d_dl = t0->b_dl.p;
        d_ep = c.epoch ? t0->b_ep.p : nullptr;
    }
    // counters and events of the call's own: ST_ROUTE_BAD, ev2 / ev3 and routePending are ShdStats'
    HIPCHK(t0->d_schedCnt.ensure(3 * kScheduleMax));
    DevEvents<2> ev;
    CHK(ev.create());
    HIPCHK(hipMemsetAsync(t0->d_schedCnt.p, 0, 8 * 3 * (size_t)k, st));
    HIPCHK(hipEventRecord(ev.e[0], st));
    HIPCHK(launch_route_schedule(T, c.n, d_src, d_dst, d_pay, d_sin, d_now, A, c.jumpNs, c.clamp,
                                 d_time, d_sout, d_dl, d_ep, t0->d_schedCnt.p, st));
    HIPCHK(hipEventRecord(ev.e[1], st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    ss->kernel_ms = ms;
    unsigned long long cnt[3 * kScheduleMax] = {};
    HIPCHK(hipMemcpy(cnt, t0->d_schedCnt.p, 8 * 3 * (size_t)k, hipMemcpyDeviceToHost));
    for (int e = 0; e < k; e++) {
        ss->epoch_packets[e] = (int64_t)cnt[3 * e];
        ss->epoch_delivered[e] = (int64_t)cnt[3 * e + 1];
        ss->not_routed += (int64_t)cnt[3 * e + 2];
    }
    if (c.epochCount) std::copy(cnt, cnt + 3 * k, c.epochCount);
    ss->bytes_model = c.n * (53 + (c.epoch ? 1 : 0));
    if (c.onDevice) return 0;
    std::vector<uint64_t> tim(n);
    std::vector<uint32_t> sout(n);
    std::vector<uint8_t> dl(n);
    HIPCHK(hipMemcpy(tim.data(), d_time, 8 * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sout.data(), d_sout, 4 * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dl.data(), d_dl, n, hipMemcpyDeviceToHost));
    if (c.epoch) HIPCHK(hipMemcpy(c.epoch, d_ep, n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
        c.out[i].time = tim[i];
        c.out[i].rngState = sout[i];
        if (sc[i] < 0) {  // not routed: the state after the sender's one draw
            uint32_t s = c.stateIn[i];
            (void)glibc_rand_r(&s);
            c.out[i].rngState = s;
        }
        c.out[i].delivered = dl[i];
        c.out[i]._pad[0] = c.out[i]._pad[1] = c.out[i]._pad[2] = 0;
    }
    if (bad) WARNING("%lld packets of a scheduled batch have an address that is not attached: "
                     "not routed", (long long)bad);
    return bad;
}

int64_t route_schedule(const ScheduleCall& c) {
    if (!args_ok(c)) return -1;
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<Topology*> mem = schedule_members(c.tops, c.k);
    return with_current_set(mem, c.n > 0, "scheduled tables", [&] {
        ShdScheduleStats ss{};
        ss.packets = c.n;
        ss.epochs = c.k;
        const int64_t r = schedule_locked(c, mem, &ss);
        ss.total_ms = ms_since(t0);
        c.tops[0]->scheduleStats = ss;
        return r;
    });
}

}  // namespace

}  // namespace shdtopo

extern "C" {

// ---- link failure what-if (include/shd_topology_abi.h) ----

Topology* shdtopo_derive_without(Topology* top, const int32_t* failEdge, int64_t ne,
                                 const int32_t* failVertex, int64_t nv, int32_t* err) {
    auto fail = [&](int32_t code) -> Topology* {
        if (err) *err = code;
        return nullptr;
    };
    if (err) *err = 0;
    if (!top || ne < 0 || nv < 0 || (ne > 0 && !failEdge) || (nv > 0 && !failVertex))
        return fail(-1);
    using clk = std::chrono::steady_clock;
    auto tq = clk::now();
    auto lap = [&]() {
        const auto t = clk::now();
        const double ms = std::chrono::duration<double, std::milli>(t - tq).count();
        tq = t;
        return ms;
    };
    const HostGraph& pg = top->g;
    // everything is validated on the parent's arrays before the child exists: an error allocates
    // no page-locked memory and starts no device thread
    std::vector<uint8_t> dropE((size_t)pg.E, 0), dropV((size_t)pg.V, 0);
    for (int64_t i = 0; i < ne; i++) {
        if (failEdge[i] < 0 || failEdge[i] >= pg.E) return fail(-1);
        dropE[(size_t)failEdge[i]] = 1;
    }
    for (int64_t i = 0; i < nv; i++)
        if (failVertex[i] < 0 || failVertex[i] >= pg.V) return fail(-1);
    int device = 0;
    {
        std::lock_guard<std::mutex> lk(top->buildMu);
        device = top->device;
    }
    std::vector<std::pair<uint32_t, int32_t>> hosts;
    {
        std::shared_lock<std::shared_mutex> lk(top->ipMu);
        for (int64_t i = 0; i < nv; i++)
            if (top->hostsOn[(size_t)failVertex[i]] > 0) {
                CRITICAL("vertex %d has %u hosts attached and cannot be failed", failVertex[i],
                         top->hostsOn[(size_t)failVertex[i]]);
                return fail(-2);
            }
        hosts.assign(top->virtualIP.begin(), top->virtualIP.end());
    }
    std::sort(hosts.begin(), hosts.end());
    bool anyV = !top->failedVertex.empty();
    if (anyV) dropV = top->failedVertex;  // (isolated already: their edges are gone)
    for (int64_t i = 0; i < nv; i++) {
        dropV[(size_t)failVertex[i]] = 1;
        anyV = true;
    }
    if (anyV)
        for (int64_t e = 0; e < pg.E; e++)
            if (dropV[(size_t)pg.eu[(size_t)e]] || dropV[(size_t)pg.ev[(size_t)e]])
                dropE[(size_t)e] = 1;
    const int64_t cut = cut_off_vertices(pg, dropE, dropV);
    if (cut != 0) {
        if (cut < 0)
            CRITICAL("the failing set leaves no vertex");
        else
            CRITICAL("the failing set cuts off %lld vertices: what remains must be but is not "
                     "strongly connected (partitioned networks are not modelled)",
                     (long long)cut);
        return fail(-3);
    }
    const double validateMs = lap();
    Topology* c = new Topology();
    c->device = device;
    c->abortOnError = top->abortOnError.load();
    c->lazy = top->lazy.load();
    start_device_init(c);  // the device initialises while the graph is copied and checked
    std::vector<int32_t> origin;
    derive_graph(pg, dropE, c->g, origin);
    if (!top->edgeOrigin.empty())
        for (int32_t& e : origin) e = top->edgeOrigin[(size_t)e];
    c->edgeOrigin = std::move(origin);
    c->rootE = root_edges(top);
    if (anyV) c->failedVertex = std::move(dropV);
    c->preChecked = true;
    const double copyMs = lap();
    c = finish_new(c);
    if (!c) return fail(-1);
    if (!getenv("SHDTOPO_NO_LOAD_PREP")) start_graph_prep(c, true);
    const double checkMs = lap();
    for (const auto& h : hosts) do_attach(c, h.first, h.second, nullptr, nullptr);
    MESSAGE("derived topology without %lld edges: validation and connectivity %.1f, copy %.1f, "
            "graph checks %.1f, %zu hosts carried over %.1f ms",
            (long long)(pg.E - c->g.E), validateMs, copyMs, checkMs, hosts.size(), lap());
    return c;
}

int64_t shdtopo_edge_origin(Topology* top, int32_t* origin, int64_t cap) {
    if (!top) return -1;
    const int64_t E = top->g.E;
    if (origin && cap >= E) {
        if (top->edgeOrigin.empty())
            for (int64_t e = 0; e < E; e++) origin[e] = (int32_t)e;
        else
            memcpy(origin, top->edgeOrigin.data(), 4 * (size_t)E);
    }
    return E;
}

int64_t shdtopo_table_diff(Topology* a, Topology* b, ShdTableChange* out, int64_t cap,
                           uint64_t kindCount[4], uint32_t* rowChanged, double* rowWorstRise,
                           int32_t* rowWorstCol) {
    if (!a || !b || cap < 0 || (cap > 0 && !out)) return -1;
    const auto t0 = std::chrono::steady_clock::now();
    return with_current_pair(a, b, true, "tables", [&] {
        ShdDiffStats ds{};
        const int64_t total = diff_locked(a, b, out, cap, kindCount, rowChanged, rowWorstRise,
                                          rowWorstCol, &ds);
        ds.changed = total < 0 ? 0 : total;
        ds.total_ms = ms_since(t0);
        a->diffStats = ds;
        return total;
    });
}

int shdtopo_table_diff_stats(Topology* a, ShdDiffStats* out) {
    return copy_stats(a, &_Topology::diffStats, out);
}

// ---- flow impact (include/shd_topology_abi.h) ----

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

// ---- load shift (include/shd_topology_abi.h) ----

int64_t shdtopo_load_shift(Topology* a, Topology* b, const uint32_t* srcIP, const uint32_t* dstIP,
                           const uint64_t* weight, int64_t n, ShdLoadChange* out, int64_t cap,
                           ShdShiftTotals* totals) {
    return load_shift(a, b, srcIP, dstIP, weight, n, out, cap, totals);
}

int shdtopo_load_shift_stats(Topology* a, ShdShiftStats* out) {
    const int r = copy_stats(a, &_Topology::shiftStats, out);
    if (!r) out->tile_entries = shift_tile_entries();
    return r;
}

// ---- route schedule (include/shd_topology_abi.h) ----

int64_t shdtopo_route_schedule_device(Topology* const* tops, const uint64_t* fromNs, int k,
                                      const int32_t* d_srcCol, const int32_t* d_dstCol,
                                      const uint32_t* d_payload, const uint32_t* d_stateIn,
                                      const uint64_t* d_now, int64_t n, uint64_t jumpNs, int clamp,
                                      uint64_t* d_time, uint32_t* d_stateOut, uint8_t* d_delivered,
                                      uint8_t* d_epoch, uint64_t* epochCount, void* stream) {
    ScheduleCall c;
    c.tops = tops;
    c.fromNs = fromNs;
    c.k = k;
    c.onDevice = true;
    c.src = d_srcCol;
    c.dst = d_dstCol;
    c.payload = d_payload;
    c.stateIn = d_stateIn;
    c.now = d_now;
    c.n = n;
    c.jumpNs = jumpNs;
    c.clamp = clamp;
    c.d_time = d_time;
    c.d_stateOut = d_stateOut;
    c.d_delivered = d_delivered;
    c.epoch = d_epoch;
    c.epochCount = epochCount;
    c.stream = (hipStream_t)stream;
    return route_schedule(c);
}

int64_t shdtopo_route_schedule_vertices(Topology* const* tops, const uint64_t* fromNs, int k,
                                        const int32_t* srcVertex, const int32_t* dstVertex,
                                        const uint32_t* payloadLength, const uint32_t* rngState,
                                        const uint64_t* now, int64_t n, uint64_t jumpNs,
                                        int clampInterHost, TopoPacketOut* out, uint8_t* epoch,
                                        uint64_t* epochCount) {
    ScheduleCall c;
    c.tops = tops;
    c.fromNs = fromNs;
    c.k = k;
    c.src = srcVertex;
    c.dst = dstVertex;
    c.payload = payloadLength;
    c.stateIn = rngState;
    c.now = now;
    c.n = n;
    c.jumpNs = jumpNs;
    c.clamp = clampInterHost;
    c.out = out;
    c.epoch = epoch;
    c.epochCount = epochCount;
    return route_schedule(c);
}

int64_t shdtopo_route_schedule(Topology* const* tops, const uint64_t* fromNs, int k,
                               const TopoPacketIn* in, TopoPacketOut* out, int64_t n,
                               uint64_t jumpNs, int clampInterHost, uint8_t* epoch,
                               uint64_t* epochCount) {
    if (!schedule_ok(tops, fromNs, k) || n < 0 || (n > 0 && (!in || !out))) return -1;
    const size_t m = (size_t)n;
    std::vector<int32_t> sv(m), dv(m);
    std::vector<uint32_t> pay(m), sin(m);
    std::vector<uint64_t> now(m);
    {
        Topology* top = tops[0];
        std::shared_lock<std::shared_mutex> lk(top->ipMu);
        for (size_t i = 0; i < m; i++) {
            auto a = top->virtualIP.find(in[i].srcIP);
            auto b = top->virtualIP.find(in[i].dstIP);
            sv[i] = a == top->virtualIP.end() ? -1 : a->second;
            dv[i] = b == top->virtualIP.end() ? -1 : b->second;
            pay[i] = in[i].payloadLength;
            sin[i] = in[i].rngState;
            now[i] = in[i].now;
        }
    }
    // (n = 0: the empty vectors' data() may be NULL, which is what a window without packets gives)
    return shdtopo_route_schedule_vertices(tops, fromNs, k, sv.data(), dv.data(), pay.data(),
                                           sin.data(), now.data(), n, jumpNs, clampInterHost, out,
                                           epoch, epochCount);
}

int shdtopo_route_schedule_stats(Topology* first, ShdScheduleStats* out) {
    return copy_stats(first, &_Topology::scheduleStats, out);
}

}  // extern "C"
