// topo_monitor_host.cpp -- the link monitor (include/shd_topology_abi.h shdtopo_monitor_*; kernels
// in topo_monitor.hip): a watch set and a bin geometry kept, the hit index over the column pairs
// built once per geometry with the flow analysis' chunk driver and validated walk (topo_host.h,
// topo_flows.cpp), cumulative bins fed by packet windows.
#include "topo_host.h"

namespace shdtopo {

static_assert(sizeof(MonRec) == 16, "MonRec is one 16-B load");

// One monitor: the watch set and the bin geometry of a timeline call, kept; the hit index over
// the column pairs of the geometry it was built for; cumulative bins and counters.  The device
// parts appear with the first use of a device: a complete topology's host feeds walk h_off /
// h_rec into h_acc and never touch one; its device feeds upload that index once.
struct LinkMonitor {
    WatchSet ws;
    uint64_t t0 = 0, binNs = 0;
    int64_t nbins = 0, rows = 0;
    // the index
    bool prepared = false, devIndex = false;
    uint64_t idxSetGen = 0, idxGeomGen = 0;
    std::vector<int32_t> idxAttached;
    int64_t A = 0, nrec = 0;
    DevBuf<int64_t> d_off;
    DevBuf<MonRec> d_rec;
    std::vector<int64_t> h_off;  // complete topologies
    std::vector<MonRec> h_rec;
    // bins rows x nbins, then the outside pairs rows x 2: device (every kernel feed) + host (the
    // host walk of a complete topology); a read sums the two
    DevBuf<unsigned long long> d_acc, d_cnt;
    bool devBins = false;
    std::vector<uint64_t> h_acc;
    int64_t hcum[MN_COUNT] = {}, hlast[MN_COUNT] = {};
    int64_t unattachedCum = 0;  // of the device counters' MN_BAD: the host feeds' share
    bool lastOnDevice = false, lastHostForm = false;
    // one event: recorded by every kernel feed on its stream; ek0 / ek1 bracket the last kernel
    hipEvent_t ev = nullptr, ek0 = nullptr, ek1 = nullptr;
    hipStream_t lastStream = nullptr;
    bool pending = false, timed = false;
    DevBuf<int32_t> b_src, b_dst;  // the host feeds' staging
    DevBuf<unsigned long long> b_w, b_now;
    DevBuf<uint8_t> b_dl;
    ShdMonitorStats st{};
    ~LinkMonitor() {
        for (hipEvent_t e : {ev, ek0, ek1})
            if (e) (void)hipEventDestroy(e);
    }
    size_t nacc() const { return (size_t)rows * ((size_t)nbins + 2); }
};

std::atomic<int> g_nextMonitor{0};

LinkMonitor* monitor_of(Topology* top, int id) {
    for (auto& m : top->monitors)
        if (m.first == id) return m.second;
    return nullptr;
}

// wait for the monitor's feeds and the library's stream
int monitor_sync(Topology* top, LinkMonitor& m) {
    if (!top->devInit) return 0;
    HIPCHK(hipSetDevice(top->devId));
    if (m.pending) HIPCHK(hipEventSynchronize(m.ev));
    m.pending = false;
    HIPCHK(hipStreamSynchronize(top->stream));
    return 0;
}

void monitors_release(Topology* top) {
    for (auto& m : top->monitors) {
        (void)monitor_sync(top, *m.second);
        delete m.second;
    }
    top->monitors.clear();
}

void monitor_drop_index(LinkMonitor& m) {
    m.prepared = m.devIndex = false;
    m.d_off.release();
    m.d_rec.release();
    std::vector<int64_t>().swap(m.h_off);
    std::vector<MonRec>().swap(m.h_rec);
    m.A = m.nrec = 0;
    m.st.index_pairs = m.st.index_records = m.st.index_bytes = 0;
}

// the device side of a monitor: events, bins, counters (zeroed once)
int monitor_dev(Topology* top, LinkMonitor& m) {
    CHK(dev_init(top));
    if (m.devBins) return 0;
    if (!m.ev) HIPCHK(hipEventCreate(&m.ev));
    if (!m.ek0) HIPCHK(hipEventCreate(&m.ek0));
    if (!m.ek1) HIPCHK(hipEventCreate(&m.ek1));
    HIPCHK(m.d_acc.ensure(std::max<size_t>(1, m.nacc())));
    HIPCHK(m.d_cnt.ensure(2 * MN_COUNT));
    HIPCHK(hipMemsetAsync(m.d_acc.p, 0, 8 * std::max<size_t>(1, m.nacc()), top->stream));
    HIPCHK(hipMemsetAsync(m.d_cnt.p, 0, 8 * 2 * MN_COUNT, top->stream));
    HIPCHK(hipStreamSynchronize(top->stream));
    m.devBins = true;
    return 0;
}

// the bytes an index may take (option "monitor_index_mb")
int monitor_cap_bytes(Topology* top, bool device, double* cap) {
    *cap = 1e30;
    if (top->monitorIndexMb > 0) {
        *cap = top->monitorIndexMb * 1048576.0;
    } else if (device) {
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        *cap = (double)fr / 2;
    }
    return 0;
}

// Complete topologies, on the host as timeline_complete: every pair is one hop over the direct
// edge, entered at offset 0, arrival at ns(0.0 + latency); a self pair over the loop.  The rows
// of sources are taken a block at a time (complete_pair_eids keeps a map of its requests).
int64_t monitor_index_complete(Topology* top, LinkMonitor& m) {
    const HostGraph& g = top->g;
    const int64_t A = top->A, ne = (int64_t)m.ws.eids.size();
    double cap = 0;
    CHK(monitor_cap_bytes(top, false, &cap));
    const double offBytes = 8.0 * ((double)A * A + 1);
    if (offBytes > cap) return -5;
    m.h_off.assign((size_t)(A * A + 1), 0);
    const int64_t blk =
        std::max<int64_t>(1, std::min<int64_t>(A, (1 << 22) / std::max<int64_t>(1, A)));
    for (int64_t c0 = 0; c0 < A; c0 += blk) {
        const int64_t c1 = std::min(A, c0 + blk), n = (c1 - c0) * A;
        std::vector<int32_t> sv((size_t)n), dv((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            sv[(size_t)i] = top->attached[(size_t)(c0 + i / A)];
            dv[(size_t)i] = top->attached[(size_t)(i % A)];
        }
        const std::vector<int32_t> pe = complete_pair_eids(top, sv, dv, n);
        for (int64_t i = 0; i < n; i++) {
            m.h_off[(size_t)(c0 * A + i)] = (int64_t)m.h_rec.size();
            const int32_t e = pe[(size_t)i];
            if (e < 0) {
                m.st.broken_pairs++;
                continue;
            }
            const int32_t ke = m.ws.edge(e), kv = m.ws.vertex(dv[(size_t)i]);
            if (ke >= 0)
                m.h_rec.push_back(
                    MonRec{0, (uint32_t)(sv[(size_t)i] != g.eu[(size_t)e] ? ne + ke : ke), 0u});
            double lat = 0.0;
            lat += g.elat[(size_t)e];
            if (kv >= 0) m.h_rec.push_back(MonRec{lat_ns(lat), (uint32_t)(ne + kv), 0u});
        }
        if (offBytes + 16.0 * (double)m.h_rec.size() > cap) return -5;
        m.st.chunks++;
    }
    m.h_off[(size_t)(A * A)] = (int64_t)m.h_rec.size();
    m.st.sources = A;
    return (int64_t)m.h_rec.size();
}

// SSSP topologies: the source columns in blocks of one chunk, each block's requests (source,
// every column) -- chains as a timeline call's (chunk_chains), link load's validation, the
// crossings' count walk (records per pair, in request = pair order), the timeline's mark walk (the
// staging segments), the scans, then the fill pass of topo_monitor.hip into the block's records.
// A block's records are allocated once its count says the index still fits; the blocks are put
// together when the last one is filled.
int64_t monitor_index_replay(Topology* top, LinkMonitor& m, ChainStats& cs) {
    CHK(dev_init(top));
    const int64_t A = top->A;
    const size_t nw = m.ws.eids.size() + m.ws.vids.size();
    double cap = 0;
    CHK(monitor_cap_bytes(top, true, &cap));
    const double offBytes = 8.0 * ((double)A * A + 1);
    if (offBytes > cap) return -5;
    hipStream_t st = nullptr;
    HIPCHK(m.d_off.ensure((size_t)(A * A + 1)));

    DevWatch dw;
    Walk wk;
    DevBuf<unsigned long long> d_wcount, d_wweight, d_ccnt, d_tcnt;
    DevBuf<int64_t> d_lcnt, d_gcnt, d_goff, d_seg, d_coff;
    DevBuf<uint2> d_stage;
    std::vector<std::unique_ptr<DevBuf<MonRec>>> blocks;
    std::vector<int64_t> blockRecs;
    int64_t total = 0;
    // the first block's size is a guess: a block that turns out wider than a chunk is taken again
    int64_t B = top->traceChunk > 0 ? top->traceChunk : 256;
    for (int64_t c0 = 0; c0 < A;) {
        B = std::max<int64_t>(1, std::min<int64_t>(B, (int64_t)(1 << 25) / A));
        const int64_t c1 = std::min(A, c0 + B), n = (c1 - c0) * A;
        std::vector<int32_t> sv((size_t)n), dv((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            sv[(size_t)i] = top->attached[(size_t)(c0 + i / A)];
            dv[(size_t)i] = top->attached[(size_t)(i % A)];
        }
        ReplayReqs R;
        double ids_ms = 0;
        CHK(group_replay_requests(top, sv, dv, n, &ids_ms, false, R));
        if (R.nsrc > R.chunk) {
            B = R.chunk;
            continue;
        }
        if (!st) {
            st = top->stream;
            CHK(dw.upload(top, m.ws));
            HIPCHK(d_wcount.ensure(nw)); HIPCHK(d_wweight.ensure(nw));
            HIPCHK(d_ccnt.ensure(CR_COUNT)); HIPCHK(d_tcnt.ensure(TL_COUNT));
            HIPCHK(hipMemsetAsync(d_wcount.p, 0, 8 * nw, st));
            HIPCHK(hipMemsetAsync(d_wweight.p, 0, 8 * nw, st));
            CHK(wk.zero(st));
            HIPCHK(hipMemsetAsync(d_ccnt.p, 0, 8 * CR_COUNT, st));
            HIPCHK(hipMemsetAsync(d_tcnt.p, 0, 8 * TL_COUNT, st));
        }
        CrossWatch cw = dw.cw;
        cw.wcount = d_wcount.p;
        cw.wweight = d_wweight.p;
        const size_t nq = (size_t)n;
        if (R.nv != nq) return -3;  // (every request has both ends attached)
        CHK(wk.upload(R, nullptr, nullptr, false));  // weights of 1, uploaded when the block grows
        HIPCHK(d_lcnt.ensure(nq + 1)); HIPCHK(d_gcnt.ensure(nq + 1)); HIPCHK(d_goff.ensure(nq + 1));
        HIPCHK(d_seg.ensure(nq + 1)); HIPCHK(d_coff.ensure(nq + 1));
        HIPCHK(hipMemsetAsync(d_lcnt.p, 0, 8 * (nq + 1), st));
        HIPCHK(hipMemsetAsync(d_gcnt.p, 0, 8 * (nq + 1), st));
        HIPCHK(hipMemsetAsync(d_seg.p, 0, 8 * (nq + 1), st));
        int64_t tot = 0;
        CHK(run_chunk(top, R, 0, R.nsrc, cs, nullptr, wk.first(R, st), [&](Chunk& ck) {
            const TraceReqs& rq = ck.rq;
            unsigned long long* w = wk.d_w.p;
            int32_t* hops = wk.d_hops.p;
            CHK(wk.pairs_counted(ck, st));
            if (ck.pairs) {
                HIPCHK(launch_cross_count_pairs(R.csr, R.pc, R.ids, rq, w, hops, cw, d_lcnt.p,
                                                d_gcnt.p, d_ccnt.p, st));
                HIPCHK(launch_timeline_mark_pairs(R.csr, R.pc, R.ids, rq, hops, dw.cw, d_seg.p,
                                                  d_tcnt.p, st));
            }
            CHK(wk.validate(R, ck, st));
            if (R.nfall > 0) {
                HIPCHK(launch_cross_count(R.csr, R.ws, R.ids, rq, w, hops, cw, d_lcnt.p, d_gcnt.p,
                                          d_ccnt.p, st));
                HIPCHK(launch_timeline_mark(R.csr, R.ws, R.ids, rq, hops, dw.cw, d_seg.p, d_tcnt.p, st));
            }
            HIPCHK(trace_exclusive_scan(d_gcnt.p, d_goff.p, n + 1, st));
            HIPCHK(trace_exclusive_scan(d_seg.p, d_coff.p, n + 1, st));
            int64_t nstage = 0;
            HIPCHK(hipMemcpyAsync(&tot, d_goff.p + n, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(&nstage, d_coff.p + n, 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (offBytes + 16.0 * (double)(total + tot) > cap) return -5;
            blocks.emplace_back(new DevBuf<MonRec>());
            DevBuf<MonRec>& rec = *blocks.back();
            HIPCHK(rec.ensure((size_t)std::max<int64_t>(1, tot)));
            HIPCHK(d_stage.ensure((size_t)std::max<int64_t>(1, nstage)));
            if (ck.pairs && tot > 0)
                HIPCHK(launch_monitor_fill_pairs(R.csr, R.pc, R.ids, rq, hops, dw.cw, d_coff.p,
                                                 d_stage.p, d_goff.p, rec.p, st));
            if (R.nfall > 0 && tot > 0)
                HIPCHK(launch_monitor_fill(R.csr, R.ws, R.ids, rq, hops, dw.cw, d_coff.p, d_stage.p,
                                           d_goff.p, rec.p, st));
            HIPCHK(launch_monitor_offsets(d_goff.p, m.d_off.p + c0 * A, n + 1, total, st));
            return 0;
        }));
        blockRecs.push_back(tot);
        total += tot;
        cs.sources += R.nsrc;
        B = R.chunk;
        c0 = c1;
    }
    if (A == 0) {
        const int64_t zero = 0;
        HIPCHK(hipMemcpy(m.d_off.p, &zero, 8, hipMemcpyHostToDevice));
    }
    HIPCHK(m.d_rec.ensure((size_t)std::max<int64_t>(1, total)));
    int64_t at = 0;
    for (size_t b = 0; b < blocks.size(); b++) {
        if (blockRecs[b] > 0)
            HIPCHK(hipMemcpyAsync(m.d_rec.p + at, blocks[b]->p,
                                  sizeof(MonRec) * (size_t)blockRecs[b], hipMemcpyDeviceToDevice,
                                  top->stream));
        at += blockRecs[b];
    }
    HIPCHK(hipStreamSynchronize(top->stream));
    if (st) HIPCHK(hipMemcpy(wk.cnt, wk.d_cnt.p, 8 * LD_COUNT, hipMemcpyDeviceToHost));
    m.st.broken_pairs = wk.broken();
    m.devIndex = true;
    return total;
}

// whether the index is the current geometry's; sg: compute_geometry's result
bool monitor_index_current(Topology* top, LinkMonitor& m, uint64_t sg) {
    if (!m.prepared) return false;
    if (m.idxSetGen == sg && m.idxGeomGen == top->geomGen) return true;
    if (m.idxAttached != top->attached) return false;
    m.idxSetGen = sg;  // (the set moved and came back: the same columns)
    m.idxGeomGen = top->geomGen;
    return true;
}

int64_t monitor_prepare_locked(Topology* top, LinkMonitor& m) {
    const auto tstart = std::chrono::steady_clock::now();
    CHK(monitor_sync(top, m));
    const uint64_t sg = compute_geometry(top);
    monitor_drop_index(m);
    if (m.rows == 0) return 0;  // no watches: no index
    m.st.prepare_ms = m.st.replay_ms = m.st.kernel_ms = m.st.batch_ms = 0;
    m.st.sources = m.st.chunks = m.st.batch_sources = m.st.batch_fallback = m.st.broken_pairs = 0;
    int64_t rec = 0;
    if (top->isComplete) {
        rec = monitor_index_complete(top, m);
    } else {
        ChainStats cs;
        rec = monitor_index_replay(top, m, cs);
        cs.out(&m.st, &ShdMonitorStats::kernel_ms);
    }
    if (rec < 0) {
        monitor_drop_index(m);
        return rec;
    }
    m.prepared = true;
    m.A = top->A;
    m.nrec = rec;
    m.idxSetGen = sg;
    m.idxGeomGen = top->geomGen;
    m.idxAttached = top->attached;
    m.st.index_pairs = m.A * m.A;
    m.st.index_records = rec;
    m.st.index_bytes = 8 * (m.A * m.A + 1) + 16 * rec;
    m.st.prepares++;
    m.st.prepare_ms = std::chrono::duration<double, std::milli>(
        std::chrono::steady_clock::now() - tstart).count();
    return rec;
}

// prepared for the current geometry, or prepare: 0, or the prepare's error
int64_t monitor_ready(Topology* top, LinkMonitor& m) {
    const uint64_t sg = compute_geometry(top);
    if (monitor_index_current(top, m, sg)) return 0;
    const int64_t r = monitor_prepare_locked(top, m);
    return r < 0 ? r : 0;
}

// the index on the device for a kernel feed (a complete topology's is uploaded once)
int monitor_dev_index(Topology* top, LinkMonitor& m) {
    if (m.devIndex) return 0;
    HIPCHK(m.d_off.ensure(m.h_off.size()));
    HIPCHK(m.d_rec.ensure(std::max<size_t>(1, m.h_rec.size())));
    HIPCHK(hipMemcpy(m.d_off.p, m.h_off.data(), 8 * m.h_off.size(), hipMemcpyHostToDevice));
    if (!m.h_rec.empty())
        HIPCHK(hipMemcpy(m.d_rec.p, m.h_rec.data(), sizeof(MonRec) * m.h_rec.size(),
                         hipMemcpyHostToDevice));
    m.devIndex = true;
    return 0;
}

// One kernel feed on st: the monitor's stream protocol, the last feed's counters zeroed, the
// kernel between ek0 / ek1, the event recorded.  w32 or w64 carries the weights (or neither).
int monitor_launch(Topology* top, LinkMonitor& m, const int32_t* d_src, const int32_t* d_dst,
                   const uint32_t* w32, const unsigned long long* w64,
                   const unsigned long long* d_now, const uint8_t* d_dl, int64_t n, hipStream_t st) {
    if (m.pending && st != m.lastStream) HIPCHK(hipStreamWaitEvent(st, m.ev, 0));
    const MonIndex ix{m.d_off.p, m.d_rec.p, m.nrec, (int32_t)m.A};
    const TimeBins tb{m.d_acc.p, m.rows, m.nbins, m.t0, m.binNs};
    HIPCHK(hipMemsetAsync(m.d_cnt.p + MN_COUNT, 0, 8 * MN_COUNT, st));
    HIPCHK(hipEventRecord(m.ek0, st));
    if (w64)
        HIPCHK(launch_monitor_feed_u64(n, d_src, d_dst, w64, d_now, d_dl, ix, tb, m.d_cnt.p, st));
    else
        HIPCHK(launch_monitor_feed(n, d_src, d_dst, w32, d_now, d_dl, ix, tb, m.d_cnt.p, st));
    HIPCHK(hipEventRecord(m.ek1, st));
    HIPCHK(hipEventRecord(m.ev, st));
    m.lastStream = st;
    m.pending = m.timed = true;
    m.lastOnDevice = true;
    return 0;
}

// A host feed by columns (-1: an end that is no column).  Complete topologies walk the host index;
// the others stage the arrays, run the feed kernel and wait for it.
int64_t monitor_feed_cols(Topology* top, LinkMonitor& m, const std::vector<int32_t>& sc,
                          const std::vector<int32_t>& dc, const uint64_t* weight,
                          const uint64_t* now, const uint8_t* delivered, int64_t n) {
    m.st.feeds++;
    if (m.rows == 0 || n == 0) return 0;
    const int64_t rr = monitor_ready(top, m);
    if (rr < 0) return rr;
    m.lastHostForm = true;
    if (top->isComplete) {
        if (m.h_acc.empty()) m.h_acc.assign(m.nacc(), 0);
        int64_t* c = m.hlast;
        std::fill(c, c + MN_COUNT, (int64_t)0);
        const int64_t A = m.A;
        const int kind[3] = {MN_BEFORE, MN_IN, MN_AFTER};
        for (int64_t i = 0; i < n; i++) {
            if (delivered && !delivered[i]) {
                c[MN_SKIPPED]++;
                continue;
            }
            if (sc[(size_t)i] < 0 || dc[(size_t)i] < 0) {
                c[MN_BAD]++;
                continue;
            }
            c[MN_FED]++;
            const size_t p = (size_t)((int64_t)sc[(size_t)i] * A + dc[(size_t)i]);
            const uint64_t w = weight ? weight[i] : 1, t = now ? now[i] : 0;
            if (m.h_off[p + 1] > m.h_off[p]) c[MN_FLOWS]++;
            for (int64_t k = m.h_off[p]; k < m.h_off[p + 1]; k++) {
                // the timeline's rule on the cumulative bins
                const MonRec& rec = m.h_rec[(size_t)k];
                c[kind[bin_add(m.t0, m.binNs, m.nbins, m.h_acc.data(),
                               m.h_acc.data() + (size_t)(m.rows * m.nbins), (int64_t)rec.row,
                               t + rec.offNs, w)]]++;
            }
        }
        for (int i = 0; i < MN_COUNT; i++) m.hcum[i] += c[i];
        m.lastOnDevice = false;
        m.timed = false;
        return c[MN_IN] + c[MN_BEFORE] + c[MN_AFTER];
    }
    CHK(monitor_dev(top, m));
    hipStream_t st = top->stream;
    const size_t nn = (size_t)n;
    HIPCHK(m.b_src.ensure(nn)); HIPCHK(m.b_dst.ensure(nn));
    HIPCHK(hipMemcpyAsync(m.b_src.p, sc.data(), 4 * nn, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(m.b_dst.p, dc.data(), 4 * nn, hipMemcpyHostToDevice, st));
    if (weight) {
        HIPCHK(m.b_w.ensure(nn));
        HIPCHK(hipMemcpyAsync(m.b_w.p, weight, 8 * nn, hipMemcpyHostToDevice, st));
    }
    if (now) {
        HIPCHK(m.b_now.ensure(nn));
        HIPCHK(hipMemcpyAsync(m.b_now.p, now, 8 * nn, hipMemcpyHostToDevice, st));
    }
    if (delivered) {
        HIPCHK(m.b_dl.ensure(nn));
        HIPCHK(hipMemcpyAsync(m.b_dl.p, delivered, nn, hipMemcpyHostToDevice, st));
    }
    CHK(monitor_launch(top, m, m.b_src.p, m.b_dst.p, nullptr, weight ? m.b_w.p : nullptr,
                       now ? m.b_now.p : nullptr, delivered ? m.b_dl.p : nullptr, n, st));
    unsigned long long c[MN_COUNT] = {};
    HIPCHK(hipMemcpyAsync(c, m.d_cnt.p + MN_COUNT, 8 * MN_COUNT, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    m.pending = false;
    m.unattachedCum += (int64_t)c[MN_BAD];
    return (int64_t)(c[MN_IN] + c[MN_BEFORE] + c[MN_AFTER]);
}

// a host feed by the packets' ends (IPs or vertices; vertex: an end's vertex, < 0 = none)
template <class T, class F>
int64_t monitor_feed_ends(Topology* top, int id, const T* src, const T* dst, const uint64_t* weight,
                          const uint64_t* now, const uint8_t* delivered, int64_t n, F&& vertex) {
    if (!top || n < 0 || n > 0x7FFFFFFE) return -1;
    if (n > 0 && (!src || !dst)) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    LinkMonitor* m = monitor_of(top, id);
    if (!m) return -1;
    compute_geometry(top);
    std::vector<int32_t> sc((size_t)n), dc((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int32_t s = vertex(src[i]), d = vertex(dst[i]);
        sc[(size_t)i] = s >= 0 && s < top->g.V ? top->colOf[(size_t)s] : -1;
        dc[(size_t)i] = d >= 0 && d < top->g.V ? top->colOf[(size_t)d] : -1;
    }
    return monitor_feed_cols(top, *m, sc, dc, weight, now, delivered, n);
}

}  // namespace shdtopo

extern "C" {

int shdtopo_monitor_new(Topology* top, const int32_t* watchEdge, int64_t ne,
                        const int32_t* watchVertex, int64_t nv, uint64_t t0, uint64_t binNs,
                        int64_t nbins) {
    int64_t rows = 0;
    if (!watch_bins_ok(top, watchEdge, ne, watchVertex, nv, binNs, nbins, &rows)) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    std::unique_ptr<LinkMonitor> m(new LinkMonitor());
    if (!m->ws.init(top->g, watchEdge, ne, watchVertex, nv)) return -1;
    m->t0 = t0;
    m->binNs = binNs;
    m->nbins = nbins;
    m->rows = rows;
    const int id = g_nextMonitor.fetch_add(1);
    top->monitors.emplace_back(id, m.release());
    return id;
}

int shdtopo_monitor_free(Topology* top, int id) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    for (size_t k = 0; k < top->monitors.size(); k++)
        if (top->monitors[k].first == id) {
            (void)monitor_sync(top, *top->monitors[k].second);
            delete top->monitors[k].second;
            top->monitors.erase(top->monitors.begin() + (std::ptrdiff_t)k);
            return 0;
        }
    return -1;
}

int64_t shdtopo_monitor_prepare(Topology* top, int id) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    LinkMonitor* m = monitor_of(top, id);
    if (!m) return -1;
    return monitor_prepare_locked(top, *m);
}

int64_t shdtopo_monitor_feed(Topology* top, int id, const uint32_t* srcIP, const uint32_t* dstIP,
                             const uint64_t* weight, const uint64_t* now, const uint8_t* delivered,
                             int64_t n) {
    // both ends on a vertex of the current attached set, as a timeline call
    return monitor_feed_ends(top, id, srcIP, dstIP, weight, now, delivered, n,
                             [&](uint32_t ip) { return vertex_of_ip(top, ip); });
}

int64_t shdtopo_monitor_feed_vertices(Topology* top, int id, const int32_t* srcVertex,
                                      const int32_t* dstVertex, const uint64_t* weight,
                                      const uint64_t* now, const uint8_t* delivered, int64_t n) {
    return monitor_feed_ends(top, id, srcVertex, dstVertex, weight, now, delivered, n,
                             [](int32_t v) { return v; });
}

int shdtopo_monitor_feed_device(Topology* top, int id, const int32_t* d_srcCol,
                                const int32_t* d_dstCol, const uint32_t* d_payload,
                                const uint64_t* d_now, const uint8_t* d_delivered, int64_t n,
                                void* stream) {
    if (!top || n < 0) return -1;
    if (n > 0 && (!d_srcCol || !d_dstCol)) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    LinkMonitor* m = monitor_of(top, id);
    if (!m) return -1;
    m->st.feeds++;
    if (m->rows == 0 || n == 0) return 0;
    const int64_t rr = monitor_ready(top, *m);
    if (rr < 0) return (int)rr;
    CHK(monitor_dev(top, *m));
    CHK(monitor_dev_index(top, *m));
    m->lastHostForm = false;
    hipStream_t st = stream ? (hipStream_t)stream : top->stream;
    return monitor_launch(top, *m, d_srcCol, d_dstCol, d_payload, nullptr,
                          (const unsigned long long*)d_now, d_delivered, n, st);
}

int shdtopo_monitor_read(Topology* top, int id, uint64_t* bins, uint64_t* outside) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    LinkMonitor* m = monitor_of(top, id);
    if (!m) return -1;
    CHK(monitor_sync(top, *m));
    const size_t nacc = m->nacc(), nb = (size_t)(m->rows * m->nbins);
    std::vector<unsigned long long> acc(nacc, 0ull);
    if (m->devBins && nacc)
        HIPCHK(hipMemcpy(acc.data(), m->d_acc.p, 8 * nacc, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < m->h_acc.size(); k++) acc[k] += m->h_acc[k];
    if (bins) std::copy(acc.begin(), acc.begin() + (std::ptrdiff_t)nb, bins);
    if (outside) std::copy(acc.begin() + (std::ptrdiff_t)nb, acc.end(), outside);
    return 0;
}

int shdtopo_monitor_reset(Topology* top, int id) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    LinkMonitor* m = monitor_of(top, id);
    if (!m) return -1;
    CHK(monitor_sync(top, *m));
    if (m->devBins) {
        HIPCHK(hipMemsetAsync(m->d_acc.p, 0, 8 * std::max<size_t>(1, m->nacc()), top->stream));
        HIPCHK(hipMemsetAsync(m->d_cnt.p, 0, 8 * 2 * MN_COUNT, top->stream));
        HIPCHK(hipStreamSynchronize(top->stream));
    }
    std::fill(m->h_acc.begin(), m->h_acc.end(), (uint64_t)0);
    std::fill(m->hcum, m->hcum + MN_COUNT, (int64_t)0);
    std::fill(m->hlast, m->hlast + MN_COUNT, (int64_t)0);
    m->unattachedCum = 0;
    return 0;
}

int shdtopo_monitor_stats(Topology* top, int id, ShdMonitorStats* out) {
    if (!top || !out) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    LinkMonitor* m = monitor_of(top, id);
    if (!m) return -1;
    CHK(monitor_sync(top, *m));
    unsigned long long dc[2 * MN_COUNT] = {};
    if (m->devBins) HIPCHK(hipMemcpy(dc, m->d_cnt.p, sizeof dc, hipMemcpyDeviceToHost));
    ShdMonitorStats& s = m->st;
    if (m->timed) {  // taken lazily: the feed itself never waits
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, m->ek0, m->ek1));
        s.feed_kernel_ms = ms;
    } else {
        s.feed_kernel_ms = 0;
    }
    auto cum = [&](int i) { return m->hcum[i] + (int64_t)dc[i]; };
    s.in_range = cum(MN_IN);
    s.before = cum(MN_BEFORE);
    s.after = cum(MN_AFTER);
    s.hits = s.in_range + s.before + s.after;
    s.flows_hit = cum(MN_FLOWS);
    s.fed = cum(MN_FED);
    s.skipped_undelivered = cum(MN_SKIPPED);
    s.unattached = m->hcum[MN_BAD] + m->unattachedCum;
    s.bad_columns = (int64_t)dc[MN_BAD] - m->unattachedCum;
    auto last = [&](int i) {
        return m->lastOnDevice ? (int64_t)dc[MN_COUNT + i] : m->hlast[i];
    };
    s.last_in_range = last(MN_IN);
    s.last_before = last(MN_BEFORE);
    s.last_after = last(MN_AFTER);
    s.last_hits = s.last_in_range + s.last_before + s.last_after;
    s.last_flows_hit = last(MN_FLOWS);
    s.last_fed = last(MN_FED);
    s.last_skipped_undelivered = last(MN_SKIPPED);
    s.last_unattached = m->lastHostForm ? last(MN_BAD) : 0;
    s.last_bad_columns = m->lastHostForm ? 0 : last(MN_BAD);
    *out = s;
    return 0;
}

int64_t shdtopo_monitor_export_index(Topology* top, int id, int64_t* pairOff, int32_t* row,
                                     uint64_t* offNs, int64_t cap) {
    if (!top || cap < 0) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    LinkMonitor* m = monitor_of(top, id);
    if (!m) return -1;
    CHK(monitor_sync(top, *m));
    if (m->rows == 0) return 0;
    const int64_t rr = monitor_ready(top, *m);
    if (rr < 0) return rr;
    const int64_t nrec = m->nrec;
    if (cap < nrec) return nrec;
    const size_t noff = (size_t)(m->A * m->A + 1);
    std::vector<MonRec> rec;
    const MonRec* hr = m->h_rec.data();
    if (!top->isComplete) {
        rec.resize((size_t)nrec);
        if (nrec)
            HIPCHK(hipMemcpy(rec.data(), m->d_rec.p, sizeof(MonRec) * (size_t)nrec,
                             hipMemcpyDeviceToHost));
        hr = rec.data();
        if (pairOff) HIPCHK(hipMemcpy(pairOff, m->d_off.p, 8 * noff, hipMemcpyDeviceToHost));
    } else if (pairOff) {
        std::copy(m->h_off.begin(), m->h_off.end(), pairOff);
    }
    for (int64_t k = 0; k < nrec; k++) {
        if (row) row[k] = (int32_t)hr[k].row;
        if (offNs) offNs[k] = hr[k].offNs;
    }
    return nrec;
}

}  // extern "C"
