// topo_flows.cpp -- the flow analysis over the table's chains: route tracing, link load, link
// crossings and the link timeline (include/shd_topology_abi.h shdtopo_trace_routes,
// shdtopo_link_load, shdtopo_link_crossings, shdtopo_link_timeline).  Complete topologies are
// answered on the host from the parsed graph; the others group their requests by source
// (group_replay_requests), take the sources' chains a chunk at a time from the batch kernel's pair
// records or the heap replay (chunk_chains) and walk them with the kernels of topo_trace.hip,
// topo_load.hip, topo_cross.hip and topo_timeline.hip.  The chunk driver (run_chunk, for_chunks)
// and the validated walk (Walk) are shared with the link monitor (topo_monitor_host.cpp).
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "topo_host.h"

// ---------------------------------------------------------------------------------------------
// route tracing (include/shd_topology_abi.h shdtopo_trace_routes; kernels in topo_trace.hip)
// ---------------------------------------------------------------------------------------------
namespace shdtopo {

static_assert(sizeof(ShdRoute) == 32 && sizeof(TraceRoute) == sizeof(ShdRoute) &&
                  offsetof(ShdRoute, hops) == offsetof(TraceRoute, hops) &&
                  offsetof(ShdRoute, status) == offsetof(TraceRoute, status) &&
                  offsetof(ShdRoute, latency) == offsetof(TraceRoute, latency) &&
                  offsetof(ShdRoute, reliability) == offsetof(TraceRoute, reliability),
              "TraceRoute is the device image of ShdRoute");

ShdRoute route_blank(int status) { return ShdRoute{-1, -1, status, -1.0, -1.0}; }

// The call's offsets on the host (complete topologies): the running sum of hops + 1 over the
// traced requests in request order; a route that does not fit below cap entirely gets status 3.
int64_t place_routes_host(ShdRoute* routes, int64_t n, int64_t cap) {
    int64_t off = 0;
    for (int64_t i = 0; i < n; i++) {
        if (routes[i].status != kTraceOk) continue;
        const int64_t need = (int64_t)routes[i].hops + 1;
        if (off + need <= cap) {
            routes[i].offset = off;
        } else {
            routes[i].offset = -1;
            routes[i].status = kTraceCap;
        }
        off += need;
    }
    return off;
}

// _topology_lookupPath (shd-topology.c:835-873) with its route: one hop over the igraph_get_eid
// edge (lowest id) of the pair, the self loop for a self pair.  Host only: the parsed graph.
std::vector<int32_t> complete_pair_eids(Topology* top, const std::vector<int32_t>& sv,
                                        const std::vector<int32_t>& dv, int64_t n) {
    const HostGraph& g = top->g;
    auto key = [](int32_t a, int32_t b) { return ((uint64_t)(uint32_t)a << 32) | (uint32_t)b; };
    std::unordered_map<uint64_t, int32_t> eidOf;
    for (int64_t i = 0; i < n; i++)
        if (sv[(size_t)i] >= 0 && dv[(size_t)i] >= 0) eidOf.emplace(key(sv[(size_t)i], dv[(size_t)i]), -1);
    for (int64_t e = 0; e < g.E; e++) {
        const int32_t a = g.eu[(size_t)e], b = g.ev[(size_t)e];
        auto it = eidOf.find(key(a, b));
        if (it != eidOf.end() && it->second < 0) it->second = (int32_t)e;
        if (!g.directed) {
            it = eidOf.find(key(b, a));
            if (it != eidOf.end() && it->second < 0) it->second = (int32_t)e;
        }
    }
    std::vector<int32_t> pe((size_t)n, -1);
    for (int64_t i = 0; i < n; i++)
        if (sv[(size_t)i] >= 0 && dv[(size_t)i] >= 0) pe[(size_t)i] = eidOf[key(sv[(size_t)i], dv[(size_t)i])];
    return pe;
}

int64_t trace_complete(Topology* top, const std::vector<int32_t>& sv, const std::vector<int32_t>& dv,
                       int64_t n, ShdRoute* routes, int32_t* vertices, int32_t* edges, int64_t cap) {
    const HostGraph& g = top->g;
    const std::vector<int32_t> pe = complete_pair_eids(top, sv, dv, n);
    std::vector<int32_t> eids((size_t)n, -1);
    for (int64_t i = 0; i < n; i++) {
        const int32_t s = sv[(size_t)i], d = dv[(size_t)i];
        if (s < 0 || d < 0) {
            routes[i] = route_blank(kTraceUnattached);
            continue;
        }
        const int32_t e = pe[(size_t)i];
        if (e < 0) {  // igraph_get_eid fails (shd-topology.c:857)
            routes[i] = route_blank(kTraceBroken);
            continue;
        }
        eids[(size_t)i] = e;
        double rel = 1.0;
        rel *= (1.0 - g.vloss[(size_t)s]);
        rel *= (1.0 - g.vloss[(size_t)d]);
        double lat = 0.0;
        lat += g.elat[(size_t)e];
        rel *= (1.0 - g.eloss[(size_t)e]);
        routes[i].offset = -1;
        routes[i].hops = 1;
        routes[i].status = kTraceOk;
        routes[i].latency = lat;
        routes[i].reliability = rel;
    }
    const int64_t total = place_routes_host(routes, n, cap);
    for (int64_t i = 0; i < n; i++) {
        const int64_t o = routes[i].offset;
        if (routes[i].status != kTraceOk || o < 0) continue;
        vertices[o] = sv[(size_t)i];
        vertices[o + 1] = dv[(size_t)i];
        edges[o] = eids[(size_t)i];
        edges[o + 1] = -1;
    }
    return total;
}

// ids of the replay CSR's vertices and entries (TraceIds), once per topology: at C4 the edge ids
// are 80 MB, so the first trace uploads them, not the build.  Caller holds buildMu; the replay
// CSR is uploaded.
int ensure_trace_ids(Topology* top, double* ms) {
    if (top->traceIdsReady) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    const HostGraph& g = top->g;
    const size_t V = (size_t)g.V;
    hipStream_t st = top->stream;
    HIPCHK(top->d_tperm.ensure(V));
    HIPCHK(hipMemcpy(top->d_tperm.p, top->hp->perm.data(), 4 * V, hipMemcpyHostToDevice));
    std::vector<int32_t> se(V, -1);  // lowest-id self loop per relabelled vertex
    for (int64_t e = 0; e < g.E; e++) {
        if (g.eu[(size_t)e] != g.ev[(size_t)e]) continue;
        int32_t& x = se[(size_t)top->hp->inv[(size_t)g.eu[(size_t)e]]];
        if (x < 0) x = (int32_t)e;
    }
    HIPCHK(top->d_selfEid.ensure(V));
    HIPCHK(hipMemcpy(top->d_selfEid.p, se.data(), 4 * V, hipMemcpyHostToDevice));
    HIPCHK(top->d_reid.ensure((size_t)std::max<int64_t>(1, top->rnadj)));
    HIPCHK(launch_trace_edge_ids(g.V, g.E, top->isDirected ? 1 : 0, top->d_eu.p, top->d_ev.p,
                                 top->d_inv.p, top->d_tperm.p, top->d_rrow.p, top->d_rrec.p,
                                 top->rnadj, top->d_reid.p, st));
    HIPCHK(hipStreamSynchronize(st));
    top->traceIdsReady = true;
    *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

// Whether this call's chains may come from the batch kernel, and if so what its
// keep launches need.  The launch must compute the rows a table build of the current attached set
// would: the build's conditions for running the batch kernel at all (the allReplay rule of
// enqueue_rows), its workspace, and a relaxation copy that is usable for the current target set
// as it stands -- a trace neither prepares a target set nor restores the plain copy.  The tree
// accumulation of a link load keeps its state in the replay's records (forLoadTree): replay.
int prepare_batch_path(Topology* top, const std::vector<uint32_t>& tgt, bool forLoadTree,
                       ReplayReqs& R) {
    R.batchOk = false;
    if (!top->traceBatch || top->isComplete || forLoadTree) return 0;
    const bool dense = top->tieReplay && (top->tieDenseOpt == 1 ||
                                          (top->tieDenseOpt < 0 && top->tieDense));
    if (top->replayAll || top->hasMultiEdges || dense) return 0;
    const bool leaf = leaf_targets_on(top);
    const bool copyOk = top->adjkPlain ? !top->targetSkip
                                       : top->adjkTargets == tgt && top->adjkLeaf == leaf;
    if (!copyOk || !top->d_adjk.p || !top->d_adj.p) return 0;
    const int K = batch_k(top);
    const size_t hparN = (size_t)std::min<int64_t>(top->parHubs, 1 << 20) * K;
    if (top->slots <= 0 || top->wsK != K || top->wsRing != ring_entries(top, K) ||
        top->wsHpar < hparN || top->wsRsChunk != top->rsChunk) {
        // no workspace of this layout (released, or never built here): the next build's
        if (ensure_workspace(top, R.nsrc) != 0) {
            (void)hipGetLastError();
            return 0;
        }
        // the one thing of this call that ShdStats keeps: the workspace a later build will find
        R.keep->stats.slots = top->stats.slots;
        R.keep->stats.workspace_bytes = top->stats.workspace_bytes;
        R.keep->stats.workspace_ms = top->stats.workspace_ms;
    }
    if (top->slots <= 0) return 0;
    R.K = K;
    const int fill = (int)top->stats.batch_fill;  // consecutive groups of the build's fill
    R.kf = fill >= 1 && fill <= K ? fill : K;
    R.delta = default_delta(top);
    R.plan = batch_lds_plan(top, K);
    R.bcsr = dev_csr(top);
    R.bws = slot_ws(top);
    R.pc = PairChains{R.bws.prec, R.bws.counters, R.bws.slots, K, R.kf};
    const int64_t A = (int64_t)tgt.size();
    const std::vector<double> sh = source_shifts(top, R.srcs.data(), R.nsrc, R.delta);
    HIPCHK(R.d_tgt.ensure((size_t)std::max<int64_t>(1, A)));
    HIPCHK(R.d_srcsh.ensure((size_t)R.nsrc));
    HIPCHK(R.d_bst.ensure(ST_COUNT));
    HIPCHK(hipMemcpy(R.d_tgt.p, tgt.data(), 4 * (size_t)A, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(R.d_srcsh.p, sh.data(), 8 * (size_t)R.nsrc, hipMemcpyHostToDevice));
    const std::vector<double> hs = source_h0_seeds(top, R.srcs.data(), R.nsrc);
    HIPCHK(R.d_h0seed.ensure((size_t)R.nsrc));
    HIPCHK(hipMemcpy(R.d_h0seed.p, hs.data(), 8 * (size_t)R.nsrc, hipMemcpyHostToDevice));
    if (leaf) {  // the build's leaf-target records: the keep launch resolves the same targets so
        CHK(ensure_leaf_targets(top, tgt, R.d_tgt.p, top->stream));
        R.bws.tleaf = top->d_tleaf.p;
    }
    R.batchOk = true;
    return 0;
}

int group_replay_requests(Topology* top, const std::vector<int32_t>& sv,
                          const std::vector<int32_t>& dv, int64_t n, double* ids_ms,
                          bool forLoadTree, ReplayReqs& R) {
    CHK(dev_init(top));
    CHK(collect_row_stats(top));  // the last build's counters are read before the replay is reused
    R.keep.reset(new TraceKeep(top));
    CHK(upload_csr(top));
    CHK(upload_replay(top));
    CHK(ensure_trace_ids(top, ids_ms));
    hipStream_t st = top->stream;
    const std::vector<int32_t>& inv = top->hp->inv;

    std::vector<uint32_t>& order = R.order;
    for (int64_t i = 0; i < n; i++)
        if (sv[(size_t)i] >= 0 && dv[(size_t)i] >= 0) order.push_back((uint32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return inv[(size_t)sv[a]] < inv[(size_t)sv[b]];
    });
    const size_t nv = R.nv = order.size();
    std::vector<uint32_t>& srcs = R.srcs;
    std::vector<uint32_t>& srcStart = R.srcStart;
    std::vector<uint32_t> rsi(nv), rsrc(nv), rdst(nv);
    for (size_t q = 0; q < nv; q++) {
        const uint32_t s = (uint32_t)inv[(size_t)sv[order[q]]];
        if (srcs.empty() || srcs.back() != s) {
            srcs.push_back(s);
            srcStart.push_back((uint32_t)q);
        }
        rsi[q] = (uint32_t)srcs.size() - 1u;
        rsrc[q] = s;
        rdst[q] = (uint32_t)inv[(size_t)dv[order[q]]];
    }
    srcStart.push_back((uint32_t)nv);
    const int nsrc = R.nsrc = (int)srcs.size();

    // the table build's target set: the chains are the table's chains
    CHK(ensure_replay_ws(top, nsrc));
    const int64_t A = top->A;
    std::vector<uint32_t> tgt((size_t)A);
    for (int64_t i = 0; i < A; i++) tgt[(size_t)i] = (uint32_t)inv[(size_t)top->attached[(size_t)i]];
    CHK(upload_target_bits(top, tgt, st));
    R.csr = replay_csr(top);
    R.ws = replay_ws(top);
    CHK(prepare_batch_path(top, tgt, forLoadTree, R));
    // a chunk's sources fit the replay's slots and, on the batch path, one batch per batch slot
    int chunk = R.ws.slots;
    if (R.batchOk)
        chunk = (int)std::min<int64_t>(chunk, (int64_t)R.bws.slots * R.kf);
    if (top->traceChunk > 0) chunk = std::min(chunk, top->traceChunk);
    if (chunk < 1) return -3;
    R.chunk = chunk;
    std::vector<uint32_t> rslot(nv);
    for (size_t q = 0; q < nv; q++) rslot[q] = rsi[q] % (uint32_t)chunk;
    for (int s0 = 0; s0 < nsrc; s0 += chunk)
        R.mmax = std::max<size_t>(R.mmax, srcStart[(size_t)std::min(nsrc, s0 + chunk)] - srcStart[(size_t)s0]);

    HIPCHK(R.d_srcs.ensure((size_t)nsrc));
    HIPCHK(R.d_rslot.ensure(nv)); HIPCHK(R.d_rsrc.ensure(nv)); HIPCHK(R.d_rdst.ensure(nv));
    HIPCHK(R.d_ridx.ensure(nv));
    HIPCHK(R.d_st.ensure(ST_COUNT));
    if (R.batchOk) {
        HIPCHK(R.d_rmap.ensure((size_t)chunk));
        HIPCHK(R.d_fsrcs.ensure((size_t)chunk));
        HIPCHK(R.d_rowflag.ensure((size_t)chunk));
        HIPCHK(R.d_broken.ensure((size_t)chunk));
    }
    HIPCHK(hipMemcpy(R.d_srcs.p, srcs.data(), 4 * (size_t)nsrc, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(R.d_rslot.p, rslot.data(), 4 * nv, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(R.d_rsrc.p, rsrc.data(), 4 * nv, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(R.d_rdst.p, rdst.data(), 4 * nv, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(R.d_ridx.p, order.data(), 4 * nv, hipMemcpyHostToDevice));
    CHK(R.ev.create());
    R.ids = TraceIds{top->d_tperm.p, top->d_reid.p, top->d_selfEid.p};
    return 0;
}

// Sources [s0, s1) of R replayed in slots 0 .. s1 - s0 - 1 (the trace launch: the vertex records
// stay for the walks); R.ev.e[0] and e[1] bracket the launch.
int launch_replay_chunk(Topology* top, ReplayReqs& R, int s0, int s1) {
    hipStream_t st = top->stream;
    HIPCHK(hipMemsetAsync(R.d_st.p, 0, sizeof(unsigned long long) * ST_COUNT, st));
    HIPCHK(hipEventRecord(R.ev.e[0], st));
    HIPCHK(launch_heap_replay_trace(R.csr, R.ws, R.d_srcs.p + s0, s1 - s0, R.d_st.p, st));
    HIPCHK(hipEventRecord(R.ev.e[1], st));
    return 0;
}

// The chains of chunk [s0, s1) of R's sources, *rq its requests.  Without the batch path: the
// replay of every source, as launch_replay_chunk.  With it:
//   keep launch of the chunk's sources (ev 3 / 4), its row flags and ST_ERRORS read back;
//   rmap: an unflagged source is served from its batch slot's pair records, a flagged one -- the
//     rows a table build replays -- gets a replay slot;
//   pairs1(rq): the caller's first pass over the pair records (the trace's count, the walks'
//     validation; ev 5 / 6), which marks the sources with a broken requested chain in
//     R.d_broken.  Only a launch that counted errors can have one: then the marks are read, those
//     sources join the replay list and pairs1 runs once more without them;
//   the replay of the listed sources in slots 0 .. nfall - 1 (ev 0 / 1).
// On return rq carries rmap, R.nfall says how many sources were replayed (their first pass is
// the caller's), and the times and counts are added to cs.
template <class F>
int chunk_chains(Topology* top, ReplayReqs& R, int s0, int s1, TraceReqs* rq, F&& pairs1,
                 ChainStats& cs) {
    hipStream_t st = top->stream;
    R.mixed = false;
    if (!R.batchOk) {
        R.nfall = s1 - s0;
        return launch_replay_chunk(top, R, s0, s1);
    }
    const int ns = s1 - s0;
    R.mixed = true;
    HIPCHK(hipMemsetAsync(R.d_bst.p, 0, sizeof(unsigned long long) * ST_COUNT, st));
    HIPCHK(hipMemsetAsync(R.d_rowflag.p, 0, (size_t)ns, st));
    HIPCHK(hipMemsetAsync(R.d_broken.p, 0, (size_t)ns, st));
    CHK(hub_rows_ready(top, R.plan.H, st));
    SlotWs ws = R.bws;
    ws.rowflag = R.d_rowflag.p;
    HIPCHK(hipEventRecord(R.ev.e[3], st));
    HIPCHK(launch_sssp_batch_keep(R.K, R.bcsr, ws, R.d_srcs.p + s0, R.d_srcsh.p + s0,
                                  R.d_h0seed.p + s0, ns, R.kf, R.d_tgt.p, (int)top->A, R.delta, R.plan, top->iterGuard,
                                  R.d_bst.p, st));
    HIPCHK(hipEventRecord(R.ev.e[4], st));
    std::vector<uint8_t> fl((size_t)ns), br((size_t)ns, 0);
    unsigned long long bst[ST_OVERFLOW + 1] = {};
    HIPCHK(hipMemcpyAsync(fl.data(), R.d_rowflag.p, (size_t)ns, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(bst, R.d_bst.p, sizeof bst, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, R.ev.e[3], R.ev.e[4]));
    cs.batch_ms += ms;
    // a launch that overflowed a queue or tripped the iteration guard is not trusted: replay
    const bool distrust = bst[ST_OVERFLOW] != 0;
    std::vector<uint32_t> fsrc;
    auto build_map = [&]() {
        R.rmap.assign((size_t)ns, kNoReplaySlot);
        fsrc.clear();
        for (int i = 0; i < ns; i++)
            if (distrust || fl[(size_t)i] || br[(size_t)i]) {
                R.rmap[(size_t)i] = (uint32_t)fsrc.size();
                fsrc.push_back(R.srcs[(size_t)(s0 + i)]);
            }
        return hipMemcpy(R.d_rmap.p, R.rmap.data(), 4 * (size_t)ns, hipMemcpyHostToDevice);
    };
    HIPCHK(build_map());
    rq->rmap = R.d_rmap.p;
    rq->nmap = (uint32_t)ns;
    if ((int)fsrc.size() < ns) {
        HIPCHK(hipEventRecord(R.ev.e[5], st));
        CHK(pairs1(*rq));
        if (bst[ST_ERRORS]) {
            HIPCHK(hipMemcpyAsync(br.data(), R.d_broken.p, (size_t)ns, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            bool any = false;
            for (int i = 0; i < ns; i++) any |= br[(size_t)i] != 0 && R.rmap[(size_t)i] == kNoReplaySlot;
            if (any) {
                HIPCHK(build_map());
                CHK(pairs1(*rq));
            }
        }
        HIPCHK(hipEventRecord(R.ev.e[6], st));
    }
    R.nfall = (int)fsrc.size();
    cs.batch_sources += ns - R.nfall;
    cs.batch_fallback += R.nfall;
    HIPCHK(hipMemsetAsync(R.d_st.p, 0, sizeof(unsigned long long) * ST_COUNT, st));
    HIPCHK(hipEventRecord(R.ev.e[0], st));
    if (R.nfall > 0) {
        HIPCHK(hipMemcpy(R.d_fsrcs.p, fsrc.data(), 4 * fsrc.size(), hipMemcpyHostToDevice));
        HIPCHK(launch_heap_replay_trace(R.csr, R.ws, R.d_fsrcs.p, R.nfall, R.d_st.p, st));
    }
    HIPCHK(hipEventRecord(R.ev.e[1], st));
    return 0;
}
// event times of a chunk after its closing event (ev 2) and a stream sync: the replay launch (if
// one ran) and everything else but the keep launch
int chunk_times(ReplayReqs& R, ChainStats& cs) {
    float ms = 0;
    if (R.nfall > 0) {
        HIPCHK(hipEventElapsedTime(&ms, R.ev.e[0], R.ev.e[1]));
        cs.replay_ms += ms;
    }
    HIPCHK(hipEventElapsedTime(&ms, R.ev.e[1], R.ev.e[2]));
    cs.kernel_ms += ms;
    if (R.mixed && R.nfall < (int)R.rmap.size()) {
        HIPCHK(hipEventElapsedTime(&ms, R.ev.e[5], R.ev.e[6]));
        cs.kernel_ms += ms;
    }
    return 0;
}

int run_chunk(Topology* top, ReplayReqs& R, int s0, int s1, ChainStats& cs, int64_t* d_zero,
              const ChunkFn& first, const ChunkFn& body) {
    hipStream_t st = top->stream;
    Chunk ck{s0, s1, R.srcStart[(size_t)s0], 0, R.reqs(s0, s1)};
    ck.m = (size_t)ck.rq.n;
    if (d_zero) HIPCHK(hipMemsetAsync(d_zero, 0, 8 * (ck.m + 1), st));
    // (the first pass reads ck.rq: by then it carries rmap)
    CHK(chunk_chains(top, R, s0, s1, &ck.rq, [&](const TraceReqs&) { return first(ck); }, cs));
    // both chain sources write the same outputs: each takes its requests
    ck.pairs = R.mixed && R.nfall < s1 - s0;
    CHK(body(ck));
    HIPCHK(hipEventRecord(R.ev.e[2], st));
    HIPCHK(hipStreamSynchronize(st));
    CHK(chunk_times(R, cs));
    cs.chunks++;
    return 0;
}

int for_chunks(Topology* top, ReplayReqs& R, ChainStats& cs, int64_t* d_zero, const ChunkFn& first,
               const ChunkFn& body) {
    cs.sources = R.nsrc;
    for (int s0 = 0; s0 < R.nsrc; s0 += R.chunk)
        CHK(run_chunk(top, R, s0, std::min(R.nsrc, s0 + R.chunk), cs, d_zero, first, body));
    return 0;
}

int Walk::upload(const ReplayReqs& R, const uint64_t* weight, const uint64_t* now, bool times) {
    const size_t nv = R.nv;
    HIPCHK(d_hops.ensure(nv));
    if (weight || ones < nv) {
        std::vector<unsigned long long> rw(nv, 1ull);
        if (weight)
            for (size_t q = 0; q < nv; q++) rw[q] = weight[R.order[q]];
        HIPCHK(d_w.ensure(nv));
        HIPCHK(hipMemcpy(d_w.p, rw.data(), 8 * nv, hipMemcpyHostToDevice));
        ones = weight ? 0 : nv;
    }
    if (times) {
        std::vector<unsigned long long> rnow(nv, 0ull);
        if (now)
            for (size_t q = 0; q < nv; q++) rnow[q] = now[R.order[q]];
        HIPCHK(d_now.ensure(nv));
        HIPCHK(hipMemcpy(d_now.p, rnow.data(), 8 * nv, hipMemcpyHostToDevice));
    }
    return 0;
}

int Walk::zero(hipStream_t st) {
    HIPCHK(d_cnt.ensure(LD_COUNT));
    HIPCHK(d_pcnt.ensure(LD_COUNT));
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, 8 * LD_COUNT, st));
    return 0;
}

ChunkFn Walk::first(ReplayReqs& R, hipStream_t st) {
    return [this, &R, st](Chunk& ck) {
        HIPCHK(hipMemsetAsync(d_pcnt.p, 0, 8 * LD_COUNT, st));
        HIPCHK(launch_load_validate_pairs(R.csr, R.pc, ck.rq, d_w.p + ck.q0, d_hops.p + ck.q0,
                                          d_pcnt.p, R.d_broken.p, st));
        return 0;
    };
}

int Walk::pairs_counted(const Chunk& ck, hipStream_t st) {
    if (!ck.pairs) return 0;
    pcnt.emplace_back();
    HIPCHK(hipMemcpyAsync(pcnt.back().data(), d_pcnt.p, 8 * LD_COUNT, hipMemcpyDeviceToHost, st));
    return 0;
}

int Walk::validate(ReplayReqs& R, const Chunk& ck, hipStream_t st) {
    if (R.nfall > 0)
        HIPCHK(launch_load_validate(R.csr, R.ws, ck.rq, d_w.p + ck.q0, d_hops.p + ck.q0, d_cnt.p, st));
    return 0;
}

// SSSP topologies: the distinct sources in chunks -- chains from the batch kernel's pair records
// or the replay (chunk_chains) -- and the walks of the requests' chains (topo_trace.hip)
int64_t trace_replay(Topology* top, const std::vector<int32_t>& sv, const std::vector<int32_t>& dv,
                     int64_t n, ShdRoute* routes, int32_t* vertices, int32_t* edges, int64_t cap,
                     ChainStats& cs) {
    ReplayReqs R;
    CHK(group_replay_requests(top, sv, dv, n, &cs.ids_ms, false, R));
    hipStream_t st = top->stream;
    const std::vector<uint32_t>& srcStart = R.srcStart;
    const size_t nv = R.nv, mmax = R.mmax;
    const int nsrc = R.nsrc, chunk = R.chunk;
    TraceEvents& ev = R.ev;

    DevBuf<TraceRoute> d_routes;
    DevBuf<int64_t> d_gneed, d_goff, d_lneed, d_coff, d_loff;
    DevBuf<int32_t> d_outV, d_outE;
    HIPCHK(d_routes.ensure((size_t)n));
    HIPCHK(d_gneed.ensure((size_t)n + 1)); HIPCHK(d_goff.ensure((size_t)n + 1));
    HIPCHK(d_lneed.ensure(mmax + 1)); HIPCHK(d_coff.ensure(mmax + 1)); HIPCHK(d_loff.ensure(nv));
    // requests with an unattached end keep their host image; pass 1 writes the others
    for (int64_t i = 0; i < n; i++) routes[i] = route_blank(kTraceUnattached);
    HIPCHK(hipMemcpy(d_routes.p, routes, sizeof(ShdRoute) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(d_gneed.p, 0, 8 * ((size_t)n + 1), st));

    std::vector<std::unique_ptr<DevBuf<int32_t>>> stage;  // per chunk: vertices, edges
    float ms = 0;
    CHK(for_chunks(
        top, R, cs, d_lneed.p,
        [&](Chunk& ck) {
            HIPCHK(launch_route_trace_count_pairs(R.csr, R.pc, ck.rq, d_routes.p, d_lneed.p,
                                                  d_gneed.p, R.d_broken.p, st));
            return 0;
        },
        [&](Chunk& ck) {
            const TraceReqs& rq = ck.rq;
            if (R.nfall > 0)
                HIPCHK(launch_route_trace_count(R.csr, R.ws, rq, d_routes.p, d_lneed.p, d_gneed.p, st));
            HIPCHK(trace_exclusive_scan(d_lneed.p, d_coff.p, (int64_t)ck.m + 1, st));
            int64_t tot = 0;
            HIPCHK(hipMemcpy(&tot, d_coff.p + ck.m, 8, hipMemcpyDeviceToHost));
            stage.emplace_back(new DevBuf<int32_t>());
            stage.emplace_back(new DevBuf<int32_t>());
            DevBuf<int32_t>& stV = *stage[stage.size() - 2];
            DevBuf<int32_t>& stE = *stage[stage.size() - 1];
            HIPCHK(stV.ensure((size_t)std::max<int64_t>(1, tot)));
            HIPCHK(stE.ensure((size_t)std::max<int64_t>(1, tot)));
            if (ck.pairs)
                HIPCHK(launch_route_trace_write_pairs(R.csr, R.pc, R.ids, rq, d_routes.p, d_coff.p,
                                                      stV.p, stE.p, st));
            if (R.nfall > 0)
                HIPCHK(launch_route_trace_write(R.csr, R.ws, R.ids, rq, d_routes.p, d_coff.p, stV.p,
                                                stE.p, st));
            HIPCHK(hipMemcpyAsync(d_loff.p + ck.q0, d_coff.p, 8 * ck.m, hipMemcpyDeviceToDevice, st));
            return 0;
        }));

    // the call's offsets: exclusive scan in request order, then the routes that fit are copied out
    HIPCHK(hipEventRecord(ev.e[0], st));
    HIPCHK(trace_exclusive_scan(d_gneed.p, d_goff.p, n + 1, st));
    HIPCHK(launch_route_trace_place(n, d_routes.p, d_goff.p, cap, st));
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_goff.p + n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(routes, d_routes.p, sizeof(ShdRoute) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t fit = 0;  // the placed routes fill [0, fit): offsets are a running sum
    for (int64_t i = 0; i < n; i++)
        if (routes[i].status == kTraceOk && routes[i].offset >= 0)
            fit = std::max(fit, routes[i].offset + routes[i].hops + 1);
    if (fit > cap) return -3;
    if (fit > 0) {
        HIPCHK(d_outV.ensure((size_t)fit));
        HIPCHK(d_outE.ensure((size_t)fit));
        size_t c = 0;
        for (int s0 = 0; s0 < nsrc; s0 += chunk, c += 2)
            HIPCHK(launch_route_trace_scatter(R.reqs(s0, std::min(nsrc, s0 + chunk)), d_routes.p,
                                              d_loff.p + srcStart[(size_t)s0], stage[c]->p,
                                              stage[c + 1]->p, d_outV.p, d_outE.p, st));
    }
    HIPCHK(hipEventRecord(ev.e[1], st));
    if (fit > 0) {
        HIPCHK(hipMemcpyAsync(vertices, d_outV.p, 4 * (size_t)fit, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(edges, d_outE.p, 4 * (size_t)fit, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    cs.kernel_ms += ms;
    return total;
}

// ---------------------------------------------------------------------------------------------
// link load (include/shd_topology_abi.h shdtopo_link_load; kernels in topo_load.hip)
// ---------------------------------------------------------------------------------------------
// Complete topologies, on the host as trace_complete: one hop over the direct edge, a self pair
// over the loop.
int64_t load_complete(Topology* top, const std::vector<int32_t>& sv, const std::vector<int32_t>& dv,
                      const uint64_t* weight, int64_t n, uint64_t* edgeLoad, uint64_t* vertexLoad,
                      ShdLoadStats* ls) {
    const HostGraph& g = top->g;
    const std::vector<int32_t> pe = complete_pair_eids(top, sv, dv, n);
    for (int64_t i = 0; i < n; i++) {
        const int32_t s = sv[(size_t)i], d = dv[(size_t)i];
        if (s < 0 || d < 0) continue;  // counted by the caller
        const int32_t e = pe[(size_t)i];
        if (e < 0) {
            ls->broken++;
            continue;
        }
        const uint64_t w = weight ? weight[i] : 1;
        if (edgeLoad) edgeLoad[s == g.eu[(size_t)e] ? (int64_t)e : g.E + e] += w;
        if (vertexLoad) vertexLoad[d] += w;
        ls->routed++;
        ls->hop_weight += w;
    }
    return ls->routed;
}

// SSSP topologies: the distinct sources in chunks -- chains from the batch kernel's pair records
// (the per-request walk only) or the replay (chunk_chains) -- and the sums along the chains, left
// on the device in the caller's holder (topo_host.h)
int load_accumulate(Topology* top, const std::vector<int32_t>& sv, const std::vector<int32_t>& dv,
                    const uint64_t* weight, int64_t n, LoadSums& sums, ShdLoadStats* ls,
                    ChainStats& cs) {
    ReplayReqs R;
    CHK(group_replay_requests(top, sv, dv, n, &cs.ids_ms, !top->loadWalk, R));
    hipStream_t st = top->stream;
    const size_t V = (size_t)top->g.V, E = (size_t)top->g.E;

    Walk wk;
    DevBuf<unsigned long long>& d_eload = sums.d_eload;
    DevBuf<unsigned long long>& d_vout = sums.d_vout;
    DevBuf<unsigned long long> d_vload;  // by relabelled vertex: permuted into d_vout below
    HIPCHK(d_eload.ensure(2 * E));
    HIPCHK(d_vload.ensure(V));
    HIPCHK(d_vout.ensure(V));
    CHK(wk.upload(R, weight, nullptr, false));
    HIPCHK(hipMemsetAsync(d_eload.p, 0, 8 * std::max<size_t>(1, 2 * E), st));
    HIPCHK(hipMemsetAsync(d_vload.p, 0, 8 * std::max<size_t>(1, V), st));
    HIPCHK(hipMemsetAsync(d_vout.p, 0, 8 * std::max<size_t>(1, V), st));
    CHK(wk.zero(st));
    const LoadAcc acc{d_eload.p, d_vload.p, (int64_t)E, top->d_eu.p};

    CHK(for_chunks(top, R, cs, nullptr, wk.first(R, st), [&](Chunk& ck) {
        const TraceReqs& rq = ck.rq;
        unsigned long long* w = wk.d_w.p + ck.q0;
        int32_t* hops = wk.d_hops.p + ck.q0;
        CHK(wk.pairs_counted(ck, st));
        if (ck.pairs) HIPCHK(launch_load_walk_pairs(R.csr, R.pc, R.ids, rq, w, hops, acc, st));
        CHK(wk.validate(R, ck, st));
        if (R.nfall > 0 && top->loadWalk) {
            HIPCHK(launch_load_walk(R.csr, R.ws, R.ids, rq, w, hops, acc, st));
        } else if (R.nfall > 0) {
            HIPCHK(launch_load_reset(R.csr, R.ws, ck.s1 - ck.s0, st));
            HIPCHK(launch_load_claim(R.csr, R.ws, R.ids, rq, w, hops, acc, wk.d_cnt.p, st));
            HIPCHK(launch_load_push(R.csr, R.ws, R.ids, rq, hops, acc, st));
        }
        return 0;
    }));

    float ms = 0;
    HIPCHK(hipEventRecord(R.ev.e[0], st));
    HIPCHK(launch_load_permute((int64_t)V, R.ids.perm, d_vload.p, d_vout.p, st));
    HIPCHK(hipEventRecord(R.ev.e[1], st));
    HIPCHK(hipMemcpyAsync(wk.cnt, wk.d_cnt.p, 8 * LD_COUNT, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventElapsedTime(&ms, R.ev.e[0], R.ev.e[1]));
    cs.kernel_ms += ms;
    ls->routed = wk.routed();
    ls->broken = wk.broken();
    ls->hop_weight = wk.total(LD_HOPW);
    ls->tree_vertices = (int64_t)wk.total(LD_TREE);
    return 0;
}

// the copy-out of a link load: the accumulated sums to the caller's arrays
int load_copy_out(Topology* top, const LoadSums& sums, uint64_t* edgeLoad, uint64_t* vertexLoad) {
    hipStream_t st = top->stream;
    const size_t V = (size_t)top->g.V, E = (size_t)top->g.E;
    if (edgeLoad && E)
        HIPCHK(hipMemcpyAsync(edgeLoad, sums.d_eload.p, 8 * 2 * E, hipMemcpyDeviceToHost, st));
    if (vertexLoad && V)
        HIPCHK(hipMemcpyAsync(vertexLoad, sums.d_vout.p, 8 * V, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// ---------------------------------------------------------------------------------------------
// link crossings (include/shd_topology_abi.h shdtopo_link_crossings; kernels in topo_cross.hip)
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(ShdCrossing) == 16 && sizeof(CrossRec) == sizeof(ShdCrossing) &&
                  offsetof(ShdCrossing, flow) == offsetof(CrossRec, flow) &&
                  offsetof(ShdCrossing, watch) == offsetof(CrossRec, watch) &&
                  offsetof(ShdCrossing, hop) == offsetof(CrossRec, hop) &&
                  offsetof(ShdCrossing, reverse) == offsetof(CrossRec, reverse),
              "CrossRec is the device image of ShdCrossing");

// the device image of a watch set (DevWatch, topo_host.h)
int DevWatch::upload(Topology* top, const WatchSet& wset) {
    const size_t V = (size_t)top->g.V, E = (size_t)top->g.E;
    const size_t ne = wset.eids.size(), nvw = wset.vids.size();
    std::vector<uint32_t> ebits(E / 32 + 1, 0u), vbits(V / 32 + 1, 0u);
    for (int32_t e : wset.eids) ebits[(size_t)e >> 5] |= 1u << (e & 31);
    std::vector<std::pair<int32_t, int32_t>> rv(nvw);
    for (size_t k = 0; k < nvw; k++) {
        const int32_t x = top->hp->inv[(size_t)wset.vids[k]];
        vbits[(size_t)x >> 5] |= 1u << (x & 31);
        rv[k] = {x, wset.vidx[k]};
    }
    std::sort(rv.begin(), rv.end());
    std::vector<int32_t> vids(nvw), vidx(nvw);
    for (size_t k = 0; k < nvw; k++) {
        vids[k] = rv[k].first;
        vidx[k] = rv[k].second;
    }
    HIPCHK(d_ebits.ensure(ebits.size())); HIPCHK(d_vbits.ensure(vbits.size()));
    HIPCHK(d_eids.ensure(std::max<size_t>(1, ne))); HIPCHK(d_eidx.ensure(std::max<size_t>(1, ne)));
    HIPCHK(d_vids.ensure(std::max<size_t>(1, nvw))); HIPCHK(d_vidx.ensure(std::max<size_t>(1, nvw)));
    HIPCHK(hipMemcpy(d_ebits.p, ebits.data(), 4 * ebits.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_vbits.p, vbits.data(), 4 * vbits.size(), hipMemcpyHostToDevice));
    if (ne) {
        HIPCHK(hipMemcpy(d_eids.p, wset.eids.data(), 4 * ne, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_eidx.p, wset.eidx.data(), 4 * ne, hipMemcpyHostToDevice));
    }
    if (nvw) {
        HIPCHK(hipMemcpy(d_vids.p, vids.data(), 4 * nvw, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_vidx.p, vidx.data(), 4 * nvw, hipMemcpyHostToDevice));
    }
    cw = CrossWatch{d_ebits.p, d_vbits.p, d_eids.p,   d_eidx.p,     d_vids.p,
                    d_vidx.p,  (int32_t)ne, (int32_t)nvw, (int64_t)E, top->d_eu.p};
    return 0;
}

// Complete topologies, on the host as load_complete: one hop (hop 0) over the direct edge, a self
// pair over the loop; the edge record before the vertex record.
int64_t cross_complete(Topology* top, const std::vector<int32_t>& sv, const std::vector<int32_t>& dv,
                       const uint64_t* weight, int64_t n, const WatchSet& ws, int64_t* flowOffset,
                       ShdCrossing* out, int64_t cap, uint64_t* watchCount, uint64_t* watchWeight,
                       ShdCrossStats* cs) {
    const HostGraph& g = top->g;
    const std::vector<int32_t> pe = complete_pair_eids(top, sv, dv, n);
    int64_t off = 0;
    for (int64_t i = 0; i < n; i++) {
        if (flowOffset) flowOffset[i] = off;
        const int32_t s = sv[(size_t)i], d = dv[(size_t)i];
        if (s < 0 || d < 0) continue;  // counted by the caller
        const int32_t e = pe[(size_t)i];
        if (e < 0) {
            cs->broken++;
            continue;
        }
        cs->routed++;
        const uint64_t w = weight ? weight[i] : 1;
        ShdCrossing rec[2];
        int m = 0;
        const int32_t ke = ws.edge(e), kv = ws.vertex(d);
        if (ke >= 0) rec[m++] = ShdCrossing{(int32_t)i, ke, 0, s != g.eu[(size_t)e] ? 1 : 0};
        if (kv >= 0) rec[m++] = ShdCrossing{(int32_t)i, kv, 0, 0};
        for (int k = 0; k < m; k++) {
            if (watchCount) watchCount[rec[k].watch]++;
            if (watchWeight) watchWeight[rec[k].watch] += w;
            if (off + m <= cap) out[off + k] = rec[k];
        }
        if (m > 0) cs->flows_hit++;
        off += m;
    }
    if (flowOffset) flowOffset[n] = off;
    return off;
}

// SSSP topologies: the distinct sources in chunks -- chains from the batch kernel's pair records
// or the replay (chunk_chains), whatever "load_walk" says -- link load's validation, then the
// count and write walks of topo_cross.hip; the records are staged per chunk and placed once the
// last chunk is walked (the structure of trace_replay)
int64_t cross_replay(Topology* top, const std::vector<int32_t>& sv, const std::vector<int32_t>& dv,
                     const uint64_t* weight, int64_t n, const WatchSet& wset, int64_t* flowOffset,
                     ShdCrossing* out, int64_t cap, uint64_t* watchCount, uint64_t* watchWeight,
                     ShdCrossStats* xs, ChainStats& cs) {
    ReplayReqs R;
    CHK(group_replay_requests(top, sv, dv, n, &cs.ids_ms, false, R));
    hipStream_t st = top->stream;
    const size_t nv = R.nv, mmax = R.mmax;
    const size_t ne = wset.eids.size(), nvw = wset.vids.size(), nw = ne + nvw;

    DevWatch dw;
    CHK(dw.upload(top, wset));
    Walk wk;
    DevBuf<unsigned long long> d_wcount, d_wweight, d_ccnt;
    DevBuf<int64_t> d_gcnt, d_goff, d_lcnt, d_coff, d_loff;
    HIPCHK(d_wcount.ensure(nw)); HIPCHK(d_wweight.ensure(nw));
    HIPCHK(hipMemsetAsync(d_wcount.p, 0, 8 * nw, st));
    HIPCHK(hipMemsetAsync(d_wweight.p, 0, 8 * nw, st));
    CrossWatch cw = dw.cw;
    cw.wcount = d_wcount.p;
    cw.wweight = d_wweight.p;

    HIPCHK(d_ccnt.ensure(CR_COUNT));
    HIPCHK(d_gcnt.ensure((size_t)n + 1)); HIPCHK(d_goff.ensure((size_t)n + 1));
    HIPCHK(d_lcnt.ensure(mmax + 1)); HIPCHK(d_coff.ensure(mmax + 1)); HIPCHK(d_loff.ensure(nv));
    CHK(wk.upload(R, weight, nullptr, false));
    CHK(wk.zero(st));
    HIPCHK(hipMemsetAsync(d_ccnt.p, 0, 8 * CR_COUNT, st));
    // requests with an unattached end have no records; the count pass writes the others
    HIPCHK(hipMemsetAsync(d_gcnt.p, 0, 8 * ((size_t)n + 1), st));

    std::vector<std::unique_ptr<DevBuf<CrossRec>>> stage;  // per chunk
    float ms = 0;
    CHK(for_chunks(
        top, R, cs, d_lcnt.p, wk.first(R, st),
        [&](Chunk& ck) {
            const TraceReqs& rq = ck.rq;
            unsigned long long* w = wk.d_w.p + ck.q0;
            int32_t* hops = wk.d_hops.p + ck.q0;
            CHK(wk.pairs_counted(ck, st));
            if (ck.pairs)
                HIPCHK(launch_cross_count_pairs(R.csr, R.pc, R.ids, rq, w, hops, cw, d_lcnt.p,
                                                d_gcnt.p, d_ccnt.p, st));
            CHK(wk.validate(R, ck, st));
            if (R.nfall > 0)
                HIPCHK(launch_cross_count(R.csr, R.ws, R.ids, rq, w, hops, cw, d_lcnt.p, d_gcnt.p,
                                          d_ccnt.p, st));
            HIPCHK(trace_exclusive_scan(d_lcnt.p, d_coff.p, (int64_t)ck.m + 1, st));
            int64_t tot = 0;
            HIPCHK(hipMemcpy(&tot, d_coff.p + ck.m, 8, hipMemcpyDeviceToHost));
            stage.emplace_back(new DevBuf<CrossRec>());
            DevBuf<CrossRec>& stg = *stage.back();
            HIPCHK(stg.ensure((size_t)std::max<int64_t>(1, tot)));
            if (ck.pairs && tot > 0)
                HIPCHK(launch_cross_write_pairs(R.csr, R.pc, R.ids, rq, hops, cw, d_coff.p, stg.p, st));
            if (R.nfall > 0 && tot > 0)
                HIPCHK(launch_cross_write(R.csr, R.ws, R.ids, rq, hops, cw, d_coff.p, stg.p, st));
            HIPCHK(hipMemcpyAsync(d_loff.p + ck.q0, d_coff.p, 8 * ck.m, hipMemcpyDeviceToDevice, st));
            return 0;
        }));

    // the call's offsets: exclusive scan in request order, then the flows that fit are copied out
    HIPCHK(hipEventRecord(R.ev.e[0], st));
    HIPCHK(trace_exclusive_scan(d_gcnt.p, d_goff.p, n + 1, st));
    std::vector<int64_t> goff((size_t)n + 1);
    HIPCHK(hipMemcpy(goff.data(), d_goff.p, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost));
    const int64_t total = goff[(size_t)n];
    // offsets ascend: the flows written are those ending at or below cap, and fill [0, fit)
    const int64_t fit =
        *(std::upper_bound(goff.begin(), goff.end(), std::min(cap, total)) - 1);
    DevBuf<CrossRec> d_out;
    if (fit > 0) {
        HIPCHK(d_out.ensure((size_t)fit));
        size_t c = 0;
        for (int s0 = 0; s0 < R.nsrc; s0 += R.chunk, c++)
            HIPCHK(launch_cross_scatter(R.reqs(s0, std::min(R.nsrc, s0 + R.chunk)), d_goff.p,
                                        d_loff.p + R.srcStart[(size_t)s0], stage[c]->p, d_out.p,
                                        fit, st));
    }
    HIPCHK(hipEventRecord(R.ev.e[1], st));
    unsigned long long ccnt[CR_COUNT] = {};
    HIPCHK(hipMemcpyAsync(wk.cnt, wk.d_cnt.p, 8 * LD_COUNT, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ccnt, d_ccnt.p, 8 * CR_COUNT, hipMemcpyDeviceToHost, st));
    if (fit > 0)
        HIPCHK(hipMemcpyAsync(out, d_out.p, sizeof(ShdCrossing) * (size_t)fit, hipMemcpyDeviceToHost, st));
    if (watchCount && nw)
        HIPCHK(hipMemcpyAsync(watchCount, d_wcount.p, 8 * nw, hipMemcpyDeviceToHost, st));
    if (watchWeight && nw)
        HIPCHK(hipMemcpyAsync(watchWeight, d_wweight.p, 8 * nw, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventElapsedTime(&ms, R.ev.e[0], R.ev.e[1]));
    cs.kernel_ms += ms;
    if (flowOffset) std::copy(goff.begin(), goff.end(), flowOffset);
    xs->routed = wk.routed();
    xs->broken = wk.broken();
    xs->flows_hit = (int64_t)ccnt[CR_FLOWS];
    if ((int64_t)ccnt[CR_RECORDS] != total) return -3;
    return total;
}

// ---------------------------------------------------------------------------------------------
// link timeline (include/shd_topology_abi.h shdtopo_link_timeline; kernels in topo_timeline.hip)
// ---------------------------------------------------------------------------------------------
// where a hit lands, and its count
struct TimelineOut {
    uint64_t t0, binNs;
    int64_t nbins;
    uint64_t* bins;
    uint64_t* outside;
    void add(int64_t row, uint64_t t, uint64_t w, ShdTimelineStats* ts) const {
        ts->hits++;
        const int k = bin_add(t0, binNs, nbins, bins, outside, row, t, w);
        (k == 0 ? ts->before : k == 1 ? ts->in_range : ts->after)++;
    }
};

// Complete topologies, on the host as cross_complete: one hop over the direct edge, entered at the
// emission time; a self pair over the loop.
int64_t timeline_complete(Topology* top, const std::vector<int32_t>& sv,
                          const std::vector<int32_t>& dv, const uint64_t* weight,
                          const uint64_t* now, int64_t n, const WatchSet& ws,
                          const TimelineOut& to, ShdTimelineStats* ts) {
    const HostGraph& g = top->g;
    const int64_t ne = (int64_t)ws.eids.size();
    const std::vector<int32_t> pe = complete_pair_eids(top, sv, dv, n);
    for (int64_t i = 0; i < n; i++) {
        const int32_t s = sv[(size_t)i], d = dv[(size_t)i];
        if (s < 0 || d < 0) continue;  // counted by the caller
        const int32_t e = pe[(size_t)i];
        if (e < 0) {
            ts->broken++;
            continue;
        }
        ts->routed++;
        const uint64_t w = weight ? weight[i] : 1, t = now ? now[i] : 0;
        const int64_t h0 = ts->hits;
        const int32_t ke = ws.edge(e), kv = ws.vertex(d);
        if (ke >= 0) to.add(s != g.eu[(size_t)e] ? ne + ke : ke, t, w, ts);
        double lat = 0.0;
        lat += g.elat[(size_t)e];
        if (kv >= 0) to.add(ne + kv, t + lat_ns(lat), w, ts);
        if (ts->hits > h0) ts->flows_hit++;
    }
    return ts->hits;
}

// SSSP topologies: the distinct sources in chunks -- chains from the batch kernel's pair records
// or the replay (chunk_chains), whatever "load_walk" says -- link load's validation, then the mark
// and time walks of topo_timeline.hip; the hops of the flows with a hit are staged per chunk and
// die with it, the bins are the call's and copied out once the last chunk is walked
int64_t timeline_replay(Topology* top, const std::vector<int32_t>& sv,
                        const std::vector<int32_t>& dv, const uint64_t* weight,
                        const uint64_t* now, int64_t n, const WatchSet& wset,
                        const TimelineOut& to, ShdTimelineStats* ts, ChainStats& cs) {
    ReplayReqs R;
    CHK(group_replay_requests(top, sv, dv, n, &cs.ids_ms, false, R));
    hipStream_t st = top->stream;
    const size_t mmax = R.mmax;
    const size_t rows = 2 * wset.eids.size() + wset.vids.size();
    const size_t nacc = rows * ((size_t)to.nbins + 2);

    DevWatch dw;
    CHK(dw.upload(top, wset));
    Walk wk;
    DevBuf<unsigned long long> d_acc, d_tcnt;
    DevBuf<int64_t> d_seg, d_coff;
    DevBuf<uint2> d_stage;
    HIPCHK(d_acc.ensure(nacc));
    HIPCHK(d_tcnt.ensure(TL_COUNT));
    HIPCHK(d_seg.ensure(mmax + 1)); HIPCHK(d_coff.ensure(mmax + 1));
    CHK(wk.upload(R, weight, now, true));
    HIPCHK(hipMemsetAsync(d_acc.p, 0, 8 * nacc, st));
    CHK(wk.zero(st));
    HIPCHK(hipMemsetAsync(d_tcnt.p, 0, 8 * TL_COUNT, st));
    const TimeBins tb{d_acc.p, (int64_t)rows, to.nbins, to.t0, to.binNs};

    CHK(for_chunks(
        top, R, cs, d_seg.p, wk.first(R, st),
        [&](Chunk& ck) {
            const TraceReqs& rq = ck.rq;
            unsigned long long* w = wk.d_w.p + ck.q0;
            unsigned long long* tnow = wk.d_now.p + ck.q0;
            int32_t* hops = wk.d_hops.p + ck.q0;
            CHK(wk.pairs_counted(ck, st));
            if (ck.pairs)
                HIPCHK(launch_timeline_mark_pairs(R.csr, R.pc, R.ids, rq, hops, dw.cw, d_seg.p,
                                                  d_tcnt.p, st));
            CHK(wk.validate(R, ck, st));
            if (R.nfall > 0)
                HIPCHK(launch_timeline_mark(R.csr, R.ws, R.ids, rq, hops, dw.cw, d_seg.p, d_tcnt.p, st));
            HIPCHK(trace_exclusive_scan(d_seg.p, d_coff.p, (int64_t)ck.m + 1, st));
            int64_t tot = 0;
            HIPCHK(hipMemcpy(&tot, d_coff.p + ck.m, 8, hipMemcpyDeviceToHost));
            HIPCHK(d_stage.ensure((size_t)std::max<int64_t>(1, tot)));
            if (ck.pairs && tot > 0)
                HIPCHK(launch_timeline_time_pairs(R.csr, R.pc, R.ids, rq, w, tnow, hops, dw.cw,
                                                  d_coff.p, d_stage.p, tb, d_tcnt.p, st));
            if (R.nfall > 0 && tot > 0)
                HIPCHK(launch_timeline_time(R.csr, R.ws, R.ids, rq, w, tnow, hops, dw.cw, d_coff.p,
                                            d_stage.p, tb, d_tcnt.p, st));
            return 0;
        }));

    unsigned long long tcnt[TL_COUNT] = {};
    std::vector<unsigned long long> acc(nacc);
    HIPCHK(hipMemcpyAsync(wk.cnt, wk.d_cnt.p, 8 * LD_COUNT, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(tcnt, d_tcnt.p, 8 * TL_COUNT, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(acc.data(), d_acc.p, 8 * nacc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const size_t nb = rows * (size_t)to.nbins;
    if (nb) std::copy(acc.begin(), acc.begin() + nb, to.bins);
    if (to.outside) std::copy(acc.begin() + nb, acc.end(), to.outside);
    ts->routed = wk.routed();
    ts->broken = wk.broken();
    ts->flows_hit = (int64_t)tcnt[TL_FLOWS];
    ts->in_range = (int64_t)tcnt[TL_IN];
    ts->before = (int64_t)tcnt[TL_BEFORE];
    ts->after = (int64_t)tcnt[TL_AFTER];
    ts->staged_hops = (int64_t)tcnt[TL_STAGED];
    ts->hits = ts->in_range + ts->before + ts->after;
    return ts->hits;
}

// The requests' vertices: both ends on a vertex of the current attached set (a table column),
// else -1.  Returns the requests with both.
int64_t resolve_requests(Topology* top, const uint32_t* srcIP, const uint32_t* dstIP, int64_t n,
                         std::vector<int32_t>& sv, std::vector<int32_t>& dv) {
    sv.resize((size_t)n);
    dv.resize((size_t)n);
    int64_t nvalid = 0;
    for (int64_t i = 0; i < n; i++) {
        int32_t s = vertex_of_ip(top, srcIP[i]), d = vertex_of_ip(top, dstIP[i]);
        if (s >= 0 && (s >= top->g.V || top->colOf[(size_t)s] < 0)) s = -1;
        if (d >= 0 && (d >= top->g.V || top->colOf[(size_t)d] < 0)) d = -1;
        sv[(size_t)i] = s;
        dv[(size_t)i] = d;
        if (s >= 0 && d >= 0) nvalid++;
    }
    return nvalid;
}

bool watch_bins_ok(Topology* top, const int32_t* watchEdge, int64_t ne, const int32_t* watchVertex,
                   int64_t nv, uint64_t binNs, int64_t nbins, int64_t* rows) {
    if (!top || ne < 0 || nv < 0 || nbins < 0 || (nbins > 0 && binNs == 0)) return false;
    if ((ne > 0 && !watchEdge) || (nv > 0 && !watchVertex)) return false;
    if (ne > top->g.E || nv > top->g.V) return false;  // (more ids than there are: a duplicate)
    *rows = 2 * ne + nv;
    return !(nbins > 0 && *rows > (int64_t)0x7FFFFFFF / nbins);  // (a device buffer of rows x bins)
}

}  // namespace shdtopo

extern "C" {

int64_t shdtopo_trace_routes(Topology* top, const uint32_t* srcIP, const uint32_t* dstIP, int64_t n,
                             ShdRoute* routes, int32_t* vertices, int32_t* edges, int64_t cap) {
    if (!top || n < 0 || cap < 0 || n > 0x7FFFFFFE) return -1;
    if (n > 0 && (!srcIP || !dstIP || !routes)) return -1;
    if (cap > 0 && (!vertices || !edges)) return -1;
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(top->buildMu);
    ShdTraceStats ts{};
    ChainStats cs;
    ts.requests = n;
    compute_geometry(top);
    // both ends on a vertex of the current attached set (a table column), else status 1
    std::vector<int32_t> sv, dv;
    const int64_t nvalid = resolve_requests(top, srcIP, dstIP, n, sv, dv);
    int64_t total = 0;
    if (top->isComplete) {
        total = trace_complete(top, sv, dv, n, routes, vertices, edges, cap);
    } else if (nvalid == 0) {
        for (int64_t i = 0; i < n; i++) routes[i] = route_blank(kTraceUnattached);
    } else {
        total = trace_replay(top, sv, dv, n, routes, vertices, edges, cap, cs);
    }
    cs.out(&ts, &ShdTraceStats::trace_kernel_ms);
    ts.ids_ms = cs.ids_ms;
    ts.entries = total;
    ts.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    top->traceStats = ts;
    return total;
}

int shdtopo_trace_stats(Topology* top, ShdTraceStats* out) {
    return copy_stats(top, &_Topology::traceStats, out);
}

int64_t shdtopo_link_load(Topology* top, const uint32_t* srcIP, const uint32_t* dstIP,
                          const uint64_t* weight, int64_t n, uint64_t* edgeLoad,
                          uint64_t* vertexLoad) {
    if (!top || n < 0 || n > 0x7FFFFFFE) return -1;
    if (n > 0 && (!srcIP || !dstIP)) return -1;
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(top->buildMu);
    ShdLoadStats ls{};
    ChainStats cs;
    ls.requests = n;
    compute_geometry(top);
    // the outputs are overwritten, not accumulated into
    if (edgeLoad) std::fill(edgeLoad, edgeLoad + 2 * (size_t)top->g.E, (uint64_t)0);
    if (vertexLoad) std::fill(vertexLoad, vertexLoad + (size_t)top->g.V, (uint64_t)0);
    std::vector<int32_t> sv, dv;
    const int64_t nvalid = resolve_requests(top, srcIP, dstIP, n, sv, dv);
    ls.unattached = n - nvalid;
    int64_t routed = 0;
    if (top->isComplete) routed = load_complete(top, sv, dv, weight, n, edgeLoad, vertexLoad, &ls);
    else if (nvalid > 0) {  // the accumulation, then the copy-out
        LoadSums sums;
        int r = load_accumulate(top, sv, dv, weight, n, sums, &ls, cs);
        if (!r) r = load_copy_out(top, sums, edgeLoad, vertexLoad);
        routed = r ? r : ls.routed;
    }
    cs.out(&ls, &ShdLoadStats::load_kernel_ms);
    ls.ids_ms = cs.ids_ms;
    ls.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    top->loadStats = ls;
    return routed;
}

int shdtopo_link_load_stats(Topology* top, ShdLoadStats* out) {
    return copy_stats(top, &_Topology::loadStats, out);
}

int64_t shdtopo_link_crossings(Topology* top, const uint32_t* srcIP, const uint32_t* dstIP,
                               const uint64_t* weight, int64_t n, const int32_t* watchEdge,
                               int64_t ne, const int32_t* watchVertex, int64_t nv,
                               int64_t* flowOffset, ShdCrossing* out, int64_t cap,
                               uint64_t* watchCount, uint64_t* watchWeight) {
    if (!top || n < 0 || n > 0x7FFFFFFE || ne < 0 || nv < 0 || cap < 0) return -1;
    if (n > 0 && (!srcIP || !dstIP)) return -1;
    if ((ne > 0 && !watchEdge) || (nv > 0 && !watchVertex) || (cap > 0 && !out)) return -1;
    if (ne > top->g.E || nv > top->g.V) return -1;  // (more ids than there are: a duplicate)
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(top->buildMu);
    WatchSet ws;
    if (!ws.init(top->g, watchEdge, ne, watchVertex, nv)) return -1;
    ShdCrossStats xs{};
    ChainStats cs;
    xs.requests = n;
    compute_geometry(top);
    // the outputs are overwritten, not accumulated into
    if (flowOffset) std::fill(flowOffset, flowOffset + (size_t)n + 1, (int64_t)0);
    if (watchCount) std::fill(watchCount, watchCount + (size_t)(ne + nv), (uint64_t)0);
    if (watchWeight) std::fill(watchWeight, watchWeight + (size_t)(ne + nv), (uint64_t)0);
    std::vector<int32_t> sv, dv;
    const int64_t nvalid = resolve_requests(top, srcIP, dstIP, n, sv, dv);
    xs.unattached = n - nvalid;
    int64_t total = 0;
    if (top->isComplete)
        total = cross_complete(top, sv, dv, weight, n, ws, flowOffset, out, cap, watchCount,
                               watchWeight, &xs);
    else if (nvalid > 0 && ne + nv > 0)  // an empty watch set: nothing to walk for
        total = cross_replay(top, sv, dv, weight, n, ws, flowOffset, out, cap, watchCount,
                             watchWeight, &xs, cs);
    cs.out(&xs, &ShdCrossStats::kernel_ms);
    xs.ids_ms = cs.ids_ms;
    xs.crossings = total < 0 ? 0 : total;
    xs.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    top->crossStats = xs;
    return total;
}

int shdtopo_link_crossings_stats(Topology* top, ShdCrossStats* out) {
    return copy_stats(top, &_Topology::crossStats, out);
}

int64_t shdtopo_link_timeline(Topology* top, const uint32_t* srcIP, const uint32_t* dstIP,
                              const uint64_t* weight, const uint64_t* now, int64_t n,
                              const int32_t* watchEdge, int64_t ne, const int32_t* watchVertex,
                              int64_t nv, uint64_t t0, uint64_t binNs, int64_t nbins,
                              uint64_t* bins, uint64_t* outside) {
    int64_t rows = 0;
    if (n < 0 || n > 0x7FFFFFFE || !watch_bins_ok(top, watchEdge, ne, watchVertex, nv, binNs, nbins, &rows))
        return -1;
    if (n > 0 && (!srcIP || !dstIP)) return -1;
    if (rows * nbins > 0 && !bins) return -1;
    const auto tstart = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(top->buildMu);
    WatchSet ws;
    if (!ws.init(top->g, watchEdge, ne, watchVertex, nv)) return -1;
    ShdTimelineStats ts{};
    ChainStats cs;
    ts.requests = n;
    compute_geometry(top);
    // the outputs are overwritten, not accumulated into
    if (bins) std::fill(bins, bins + (size_t)(rows * nbins), (uint64_t)0);
    if (outside) std::fill(outside, outside + (size_t)(2 * rows), (uint64_t)0);
    std::vector<int32_t> sv, dv;
    const int64_t nvalid = resolve_requests(top, srcIP, dstIP, n, sv, dv);
    ts.unattached = n - nvalid;
    const TimelineOut to{t0, binNs, nbins, bins, outside};
    int64_t hits = 0;
    if (rows == 0) hits = 0;  // an empty watch set: nothing to walk for
    else if (top->isComplete) hits = timeline_complete(top, sv, dv, weight, now, n, ws, to, &ts);
    else if (nvalid > 0) hits = timeline_replay(top, sv, dv, weight, now, n, ws, to, &ts, cs);
    cs.out(&ts, &ShdTimelineStats::kernel_ms);
    ts.ids_ms = cs.ids_ms;
    if (hits < 0) ts.hits = 0;
    ts.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tstart).count();
    top->timelineStats = ts;
    return hits;
}

int shdtopo_link_timeline_stats(Topology* top, ShdTimelineStats* out) {
    return copy_stats(top, &_Topology::timelineStats, out);
}

int64_t shdtopo_format_route(Topology* top, const ShdRoute* r, const int32_t* vertices,
                             const int32_t* edges, char* buf, size_t cap) {
    if (!top || !r || !vertices || !edges || (cap > 0 && !buf)) return -1;
    if (r->status != kTraceOk || r->offset < 0 || r->hops < 1) return -1;
    const HostGraph& g = top->g;
    const int32_t* v = vertices + r->offset;
    const int32_t* e = edges + r->offset;
    const int64_t h = r->hops;
    for (int64_t k = 0; k <= h; k++)
        if (v[k] < 0 || v[k] >= g.V) return -1;
    for (int64_t k = 0; k < h; k++)
        if (e[k] < 0 || (int64_t)e[k] >= g.E) return -1;
    // shd-topology.c:594,644,654-656
    char num[400];
    std::string path = g.vid[(size_t)v[0]];
    for (int64_t k = 0; k < h; k++) {
        snprintf(num, sizeof num, "--[%f,%f]-->", g.elat[(size_t)e[k]], 1.0 - g.eloss[(size_t)e[k]]);
        path += num;
        path += g.vid[(size_t)v[k + 1]];
    }
    std::string out = "shortest path " + g.vid[(size_t)v[0]] + "-->" + g.vid[(size_t)v[h]];
    snprintf(num, sizeof num, " (%i-->%i) is %f ms", (int)v[0], (int)v[h], r->latency);
    out += num;
    snprintf(num, sizeof num, " with %f loss, path: ", 1.0 - r->reliability);
    out += num;
    out += path;
    if (cap > 0) {
        const size_t c = std::min(out.size(), cap - 1);
        memcpy(buf, out.data(), c);
        buf[c] = 0;
    }
    return (int64_t)out.size();
}

}  // extern "C"
