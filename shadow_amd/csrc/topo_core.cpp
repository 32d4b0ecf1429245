// topo_core.cpp -- the Topology object behind the C ABI of include/shd_topology_abi.h.
//
// Reference: src/topology/shd-topology.c (Shadow v1.11.1).  What changes against the reference:
//   * paths are not computed lazily one igraph Dijkstra at a time under a global lock
//     (shd-topology.c:673-833); the whole attached-vertex table is built on the
//     GPU on first use after the attach set settles (sssp_batch_kernel + heap_replay_kernel /
//     pair_table_complete_kernel);
//   * getters read an immutable table; the reference's first-rooted-wins cache behaviour
//     (shd-topology.c:894-915) is reproduced with per-source "materialised"
//     flags (lazy mode, default) so answers and the min-latency trajectory are bit-identical
//     for the same query sequence;
//   * attach uses a candidate index built once instead of an O(V) scan per host.
#include <arpa/inet.h>

#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <queue>
#include <unordered_set>

#include "topo_host.h"

// ---- imports from the Shadow executable (weak: absent in a standalone process) ----
extern "C" {
__attribute__((weak)) uint32_t address_toNetworkIP(Address* address);
__attribute__((weak)) double random_nextDouble(Random* random);
__attribute__((weak)) void worker_updateMinTimeJump(double minPathLatency);
// src/support/shd-logging.h:122-124 (GLogLevelFlags passed as int): Shadow's logger prefixes the
// real time, the simulated time and the host, and applies the configured log-level filter
__attribute__((weak)) void logging_log(const char* log_domain, int log_level, const char* fileName,
                                       const char* functionName, int lineNumber,
                                       const char* format, ...);
}
using namespace shdtopo;

namespace shdtopo {
// Page-locked allocations of the parsed graph's edge arrays (topo_internal.h PinnedAlloc): the
// registry tells hipHostFree from free when a buffer is released.
namespace {
std::mutex g_pinMu;
std::unordered_set<void*> g_pinned;
}  // namespace
void* pinned_alloc(size_t bytes) {
    if (bytes == 0) bytes = 1;
    void* p = nullptr;
    if (!getenv("SHDTOPO_NO_PINNED") && hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess && p) {
        std::lock_guard<std::mutex> lk(g_pinMu);
        g_pinned.insert(p);
        return p;
    }
    (void)hipGetLastError();  // no device (CPU-only use): ordinary memory
    return malloc(bytes);
}
void pinned_free(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_pinMu);
        auto it = g_pinned.find(p);
        if (it != g_pinned.end()) {
            g_pinned.erase(it);
            (void)hipHostFree(p);
            return;
        }
    }
    free(p);
}

// Standalone filter (no Shadow logger): SHDTOPO_LOG = 0 silent, 1 critical + warning (default),
// 2 + message, 3 + info
static int log_level() {
    static int lvl = [] {
        const char* e = getenv("SHDTOPO_LOG");
        return e ? atoi(e) : 1;
    }();
    return lvl;
}

void shd_log(int glevel, const char* file, const char* func, int line, const char* fmt, ...) {
    const int lvl = glevel <= kLogWarning ? 1 : (glevel == kLogMessage ? 2 : 3);
    if (!logging_log && lvl > log_level()) return;
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (logging_log) {
        logging_log("shadow", glevel, file, func, line, "%s", buf);
        return;
    }
    const char* tag = glevel == kLogCritical ? "critical"
                      : glevel == kLogWarning ? "warning"
                      : glevel == kLogMessage ? "message" : "info";
    fprintf(stderr, "[shdtopo] %s: %s\n", tag, buf);
}

uint64_t next_topology_uid() {
    static std::atomic<uint64_t> n{0};
    return n.fetch_add(1) + 1;
}

// (external linkage: topo_host.h declares what the other host units call)
void fatal_or_continue(Topology* top, const char* what) {
    CRITICAL("%s", what);
    if (top->abortOnError) abort();
}

// ---------------------------------------------------------------------------------------------
// validation (shd-topology.c:125-432)
// ---------------------------------------------------------------------------------------------
bool check_graph(Topology* top) {
    HostGraph& g = top->g;
    if (g.V == 0) {
        CRITICAL("topology has no vertices");
        return false;
    }
    // strong connectivity (igraph_is_connected(STRONG) + igraph_clusters, :134-151)
    std::vector<std::vector<int32_t>> dummy;
    std::vector<int64_t> optr((size_t)g.V + 1, 0), iptr((size_t)g.V + 1, 0);
    for (int64_t e = 0; e < g.E; e++) {
        optr[(size_t)g.eu[(size_t)e] + 1]++;
        iptr[(size_t)g.ev[(size_t)e] + 1]++;
    }
    for (int32_t v = 0; v < g.V; v++) {
        optr[(size_t)v + 1] += optr[(size_t)v];
        iptr[(size_t)v + 1] += iptr[(size_t)v];
    }
    std::vector<int32_t> oadj((size_t)g.E), iadj((size_t)g.E);
    {
        std::vector<int64_t> po(optr.begin(), optr.end() - 1), pi(iptr.begin(), iptr.end() - 1);
        for (int64_t e = 0; e < g.E; e++) {
            oadj[(size_t)po[(size_t)g.eu[(size_t)e]]++] = g.ev[(size_t)e];
            iadj[(size_t)pi[(size_t)g.ev[(size_t)e]]++] = g.eu[(size_t)e];
        }
    }
    auto reach_all = [&](bool forward, bool both) {
        std::vector<uint8_t> seen((size_t)g.V, 0);
        std::vector<int32_t> st{0};
        seen[0] = 1;
        int64_t cnt = 1;
        while (!st.empty()) {
            int32_t x = st.back();
            st.pop_back();
            auto visit = [&](const std::vector<int64_t>& ptr, const std::vector<int32_t>& adj) {
                for (int64_t i = ptr[(size_t)x]; i < ptr[(size_t)x + 1]; i++) {
                    int32_t y = adj[(size_t)i];
                    if (!seen[(size_t)y]) { seen[(size_t)y] = 1; cnt++; st.push_back(y); }
                }
            };
            if (forward || both) visit(optr, oadj);
            if (!forward || both) visit(iptr, iadj);
        }
        return cnt == g.V;
    };
    // (a derived topology: shdtopo_derive_without checked the vertices that are not failed)
    bool connected = top->preChecked ||
                     (g.directed ? (reach_all(true, false) && reach_all(false, false))
                                 : reach_all(true, true));
    if (!connected) {
        CRITICAL("topology must be but is not strongly connected");
        return false;
    }
    top->isDirected = g.directed;
    // complete <=> clique number == V (:156-165): every distinct pair adjacent (direction,
    // loops and multi-edges ignored)
    {
        std::vector<uint64_t> keys;
        keys.reserve((size_t)g.E);
        for (int64_t e = 0; e < g.E; e++) {
            uint64_t a = (uint64_t)g.eu[(size_t)e], b = (uint64_t)g.ev[(size_t)e];
            if (a == b) continue;
            if (a > b) std::swap(a, b);
            keys.push_back(a * (uint64_t)g.V + b);
        }
        std::sort(keys.begin(), keys.end());
        size_t uniq = (size_t)(std::unique(keys.begin(), keys.end()) - keys.begin());
        top->hasMultiEdges = uniq != keys.size();
        if (g.directed && top->hasMultiEdges) {  // directed: only same-direction duplicates
            keys.clear();
            for (int64_t e = 0; e < g.E; e++)
                if (g.eu[(size_t)e] != g.ev[(size_t)e])
                    keys.push_back((uint64_t)g.eu[(size_t)e] * (uint64_t)g.V + (uint64_t)g.ev[(size_t)e]);
            std::sort(keys.begin(), keys.end());
            top->hasMultiEdges = std::unique(keys.begin(), keys.end()) != keys.end();
        }
        top->isComplete = (uint64_t)uniq == (uint64_t)g.V * (uint64_t)(g.V - 1) / 2;
    }
    if (top->hasMultiEdges)
        WARNING("topology has parallel edges: igraph_get_eid picks one of them "
                "(implementation-defined); the lowest edge id is used here, and every row is "
                "computed by the exact heap replay");
    // edge latency > 0 (:312-317; the reference calls error() here)
    for (int64_t e = 0; e < g.E; e++) {
        if (g.elat[(size_t)e] <= 0) {
            CRITICAL("invalid latency %f on edge %lld", g.elat[(size_t)e], (long long)e);
            return false;
        }
    }
    MESSAGE("topology graph is %s, %s, strongly connected, %d vertices, %lld edges",
            top->isComplete ? "complete" : "incomplete",
            top->isDirected ? "directed" : "undirected", g.V, (long long)g.E);
    top->aidx.build(g, top->failedVertex.empty() ? nullptr : &top->failedVertex);
    // the edge scan (mean latency, the replay's integer-key check) belongs to loading the graph
    // too: done here, inside topology_new, it is off the first table's critical path (round 4: 24
    // ms of the attach-time preparation on C4)
    edge_scan(top);
    top->matGen.reset(new std::atomic<uint64_t>[(size_t)g.V]);
    for (int32_t v = 0; v < g.V; v++) top->matGen[(size_t)v].store(0);
    top->hostsOn.assign((size_t)g.V, 0u);
    return true;
}

Topology* finish_new(Topology* top) {
    if (!check_graph(top)) {
        topology_free(top);  // joins the device-init thread, releases the device
        return nullptr;
    }
    return top;
}

// a new Topology: its device is SHDTOPO_DEVICE (else 0) unless the "device" option changes it
Topology* new_topology(bool earlyInit) {
    Topology* top = new Topology();
    if (const char* d = getenv("SHDTOPO_DEVICE")) top->device = atoi(d);
    if (earlyInit) start_device_init(top);
    return top;
}

// ---------------------------------------------------------------------------------------------
// device setup
// ---------------------------------------------------------------------------------------------
int dev_init(Topology* top) {
    top->deviceUsed = true;  // (topology_new's background init restores it: start_device_init)
    if (top->devInit) {
        // HIP's current device is per thread: bind this engine's device for the caller
        HIPCHK(hipSetDevice(top->devId));
        return 0;
    }
    const bool trace = getenv("SHDTOPO_TRACE_INIT") != nullptr;
    auto ti = std::chrono::steady_clock::now();
    auto tmark = [&](const char* what) {
        if (!trace) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[shdtopo] dev_init %s: %.2f ms\n", what,
                std::chrono::duration<double, std::milli>(t - ti).count());
        ti = t;
    };
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        CRITICAL("no HIP device available: the routing engine runs on the GPU only "
                 "(no CPU fallback)");
        return -1;
    }
    tmark("device count");
    top->devId = top->device % n;
    HIPCHK(hipSetDevice(top->devId));
    tmark("set device");
    HIPCHK(hipStreamCreateWithFlags(&top->stream, hipStreamNonBlocking));
    tmark("stream");
    HIPCHK(hipEventCreate(&top->ev0));
    HIPCHK(hipEventCreate(&top->ev1));
    HIPCHK(hipEventCreate(&top->ev2));
    HIPCHK(hipEventCreate(&top->ev3));
    HIPCHK(hipEventCreate(&top->evr0));
    HIPCHK(hipEventCreate(&top->evr1));
    HIPCHK(hipEventCreate(&top->evp0));
    HIPCHK(hipEventCreate(&top->evp1));
    tmark("events");
    HIPCHK(top->d_stats.ensure(ST_COUNT));
    // (a build zeroes the block again; a table installed by shdtopo_bind_table* has none before
    // its first packet route adds to ST_ROUTE_BAD)
    HIPCHK(hipMemset(top->d_stats.p, 0, sizeof(unsigned long long) * ST_COUNT));
    tmark("stats buffer");
    for (hipStream_t& c : top->cstream) HIPCHK(hipStreamCreateWithFlags(&c, hipStreamNonBlocking));
    {
        // a pageable copy each way: the runtime sets up its staging buffers here (the background
        // init) rather than in the first build's or the first getter's copies
        unsigned long long h[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpy(h, top->d_stats.p, sizeof h, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(top->d_stats.p, h, sizeof h, hipMemcpyHostToDevice));
    }
    tmark("copy streams + staging");
    // the kernels' code objects, loaded here rather than by the first build's launches
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(preload_prep_module());
    tmark("prep module");
    HIPCHK(preload_batch_module());
    tmark("batch module");
    HIPCHK(preload_kernels_module());
    tmark("kernels module");
    HIPCHK(preload_replay_module());
    tmark("replay module");
    {
        // a warm-up only: a failure here costs the first build its ~12 ms, nothing else
        const hipError_t we = preload_kprime_sort(top->stream);
        if (we != hipSuccess) {
            (void)hipGetLastError();
            MESSAGE("background init: sort warm-up failed (%s); the first build pays its setup",
                    hipGetErrorString(we));
        }
    }
    tmark("first radix sort");
    top->stats.module_load_ms = std::chrono::duration<double, std::milli>(
        std::chrono::steady_clock::now() - t0).count();
    top->devInit = true;
    top->devInits++;
    return 0;
}

// Undo dev_init: the "device" option changed after topology_new's background init bound the
// default device (before the first attach).  The next dev_init binds the new device.
void dev_release(Topology* top) {
    if (!top->devInit) return;
    (void)hipSetDevice(top->devId);
    (void)hipStreamSynchronize(top->stream);
    for (hipEvent_t e : {top->ev0, top->ev1, top->ev2, top->ev3, top->evr0, top->evr1, top->evp0,
                         top->evp1})
        (void)hipEventDestroy(e);
    (void)hipStreamDestroy(top->stream);
    if (top->xstream) (void)hipStreamDestroy(top->xstream);
    for (hipStream_t& c : top->cstream) {
        if (c) (void)hipStreamDestroy(c);
        c = nullptr;
    }
    top->stream = top->xstream = nullptr;
    top->ev0 = top->ev1 = top->ev2 = top->ev3 = top->evr0 = top->evr1 = nullptr;
    top->evp0 = top->evp1 = nullptr;
    top->d_stats.release();
    top->devInit = false;
}

// topology_new's background device init (Topology::initThread): the HIP context, the library's
// stream and events and the kernels' code objects on the default device while the GraphML is
// parsed (C4: 2.8 s of parsing hide ~150 ms of device init).  Holds buildMu, so an early
// set_option or build waits for it.  No device present: nothing to do (the first build reports).
void start_device_init(Topology* top) {
    if (getenv("SHDTOPO_NO_EARLY_INIT")) return;
    top->initThread = std::thread([top]() {
        std::lock_guard<std::mutex> lk(top->buildMu);
        const auto t0 = std::chrono::steady_clock::now();
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            return;
        }
        const bool used = top->deviceUsed;
        if (dev_init(top) != 0) (void)hipGetLastError();
        top->deviceUsed = used;  // binding the default device early is not a use of it
        top->initBgMs = std::chrono::duration<double, std::milli>(
            std::chrono::steady_clock::now() - t0).count();
    });
}

HubSegs hub_segs(Topology* top) {
    HubSegs h;
    h.rows = top->hsegRows;
    h.seg = top->d_hseg.p;
    h.nseg = top->hsegN;
    h.multi = top->d_hmulti.p;
    h.nmulti = top->hmultiN;
    return h;
}

// out-rows (relaxation, kappa copy, target fixpoint) and in-rows (parent pass) of the prepared
// graph: one adjacency serves both when undirected
const uint32_t* adj_out(Topology* top) { return top->isDirected ? top->d_adjo.p : top->d_adj.p; }
const uint32_t* rowptr_in(Topology* top) {
    return top->isDirected ? top->d_rowptrIn.p : top->d_rowptr.p;
}

// segment tables of rows [0, H) of a device rowptr (host copy of its head)
int make_hub_segs(const uint32_t* d_rowptr, uint32_t H, DevBuf<uint2>& dseg,
                  DevBuf<uint4>& dmulti, uint32_t* nseg, uint32_t* nmulti, hipStream_t st) {
    std::vector<uint32_t> head((size_t)H + 1);
    HIPCHK(hipMemcpyAsync(head.data(), d_rowptr, 4 * ((size_t)H + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<uint2> seg;
    std::vector<uint4> multi;
    hub_segments(head.data(), H, seg, multi);
    dseg.release();
    dmulti.release();
    HIPCHK(dseg.ensure(seg.size()));
    HIPCHK(hipMemcpyAsync(dseg.p, seg.data(), sizeof(uint2) * seg.size(), hipMemcpyHostToDevice, st));
    if (!multi.empty()) {
        HIPCHK(dmulti.ensure(multi.size()));
        HIPCHK(hipMemcpyAsync(dmulti.p, multi.data(), sizeof(uint4) * multi.size(), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    *nseg = (uint32_t)seg.size();
    *nmulti = (uint32_t)multi.size();
    return 0;
}

int upload_csr_impl(Topology* top);
int upload_csr(Topology* top) {
    if (top->csrUploaded) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int r = upload_csr_impl(top);
    top->stats.csr_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return r;
}

// Graph preparation.  Topologies are prepared on the GPU
// (topo_prep.hip): the parsed edge arrays are copied to HBM once, and the relabel, the CSR, the
// h0 distances and tree and the kappa-sorted relaxation copy are built there; the host keeps only
// perm / inv / pi / the h0-tree parents (source ordering of the batched builds, the replay CSR).
int upload_csr_impl(Topology* top) {
    HostGraph& g = top->g;
    const int32_t V = g.V;
    using clk = std::chrono::steady_clock;
    double host_ms = 0.0, copy_ms = 0.0;
    top->hp = std::make_shared<HostPrep>();
    top->csrHostRuns++;
    const int64_t E = g.E;
    auto tstep = clk::now();
    for (double& x : top->stats.csr_step_ms) x = 0.0;
    auto step_done = [&](int i) {
        const auto t = clk::now();
        top->stats.csr_step_ms[i] = std::chrono::duration<double, std::milli>(t - tstep).count();
        tstep = t;
    };
    if (2 * E >= (int64_t)INT32_MAX || (int64_t)V >= (int64_t)1 << 30) {
        CRITICAL("topology too large for the device CSR (%d vertices, %lld edges)", V, (long long)E);
        return -7;
    }
    hipStream_t st = top->stream;
    // 1) the parsed graph to HBM (document order)
    // (kept in HBM: the heap replay's incidence CSR is built from them on the GPU too)
    DevBuf<int32_t>& eu = top->d_eu;
    DevBuf<int32_t>& ev = top->d_ev;
    DevBuf<double>& elat = top->d_elat;
    DevBuf<double>& eloss = top->d_eloss;
    DevBuf<double> vl0;
    HIPCHK(eu.ensure((size_t)E));
    HIPCHK(ev.ensure((size_t)E));
    HIPCHK(elat.ensure((size_t)E));
    HIPCHK(eloss.ensure((size_t)E));
    HIPCHK(vl0.ensure((size_t)V));
    {
        const auto tc = clk::now();
        HIPCHK(hipMemcpyAsync(eu.p, g.eu.data(), 4 * (size_t)E, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ev.p, g.ev.data(), 4 * (size_t)E, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(elat.p, g.elat.data(), 8 * (size_t)E, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(eloss.p, g.eloss.data(), 8 * (size_t)E, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(vl0.p, g.vloss.data(), 8 * (size_t)V, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        copy_ms += ms_since(tc);
    }
    step_done(0);
    // 2) degrees, relabel, rows
    DevBuf<uint32_t> deg, selfE, dperm;
    DevBuf<uint32_t>& dinv = top->d_inv;
    HIPCHK(deg.ensure((size_t)V));
    HIPCHK(selfE.ensure((size_t)V));
    int64_t nadj = 0;
    HIPCHK(prep_degrees(V, E, eu.p, ev.p, deg.p, selfE.p, &nadj, st));
    // a directed edge is one entry of its tail's out-row and one of its head's in-row
    const bool dir = top->isDirected;
    if (dir) nadj /= 2;
    const uint32_t H = (uint32_t)std::min<int64_t>(kGroupHubs, V);
    HIPCHK(dperm.ensure((size_t)V));
    HIPCHK(dinv.ensure((size_t)V));
    HIPCHK(top->d_rowptr.ensure((size_t)V + 1));
    HIPCHK(top->d_vloss.ensure((size_t)V));
    HIPCHK(top->d_selfLat.ensure((size_t)V));
    HIPCHK(top->d_selfLoss.ensure((size_t)V));
    HIPCHK(prep_relabel(V, E, H, eu.p, ev.p, deg.p, selfE.p, elat.p, eloss.p, vl0.p, dperm.p,
                        dinv.p, top->d_rowptr.p, top->d_vloss.p, top->d_selfLat.p,
                        top->d_selfLoss.p, st));
    deg.release();
    selfE.release();
    vl0.release();
    step_done(1);
    if (!dir) {
        HIPCHK(top->d_adj.ensure(4 * (size_t)nadj));
        HIPCHK(top->d_aloss.ensure((size_t)nadj));
        HIPCHK(prep_adjacency(V, E, nadj, eu.p, ev.p, dinv.p, elat.p, eloss.p, top->d_adj.p,
                              top->d_aloss.p, st));
    } else {
        // out-rows (d_rowptr counted from them, replacing prep_relabel's in + out degrees) and
        // in-rows with their losses
        HIPCHK(top->d_adjo.ensure(4 * (size_t)std::max<int64_t>(1, nadj)));
        HIPCHK(prep_adjacency(V, E, nadj, eu.p, ev.p, dinv.p, elat.p, eloss.p, top->d_adjo.p,
                              nullptr, st, kAdjOut, top->d_rowptr.p));
        HIPCHK(top->d_rowptrIn.ensure((size_t)V + 1));
        HIPCHK(top->d_adj.ensure(4 * (size_t)std::max<int64_t>(1, nadj)));
        HIPCHK(top->d_aloss.ensure((size_t)std::max<int64_t>(1, nadj)));
        HIPCHK(prep_adjacency(V, E, nadj, eu.p, ev.p, dinv.p, elat.p, eloss.p, top->d_adj.p,
                              top->d_aloss.p, st, kAdjIn, top->d_rowptrIn.p));
    }
    // the hub rows' segment tables (HubSegs) from the head of the (out-)rowptr
    {
        uint32_t ns = 0, nm = 0;
        const int r = make_hub_segs(top->d_rowptr.p, H, top->d_hseg, top->d_hmulti, &ns, &nm, st);
        if (r) return r;
        top->hsegRows = H;
        top->hsegN = ns;
        top->hmultiN = nm;
    }
    step_done(2);
    // 3) pi = d(h0, .) over the out-rows, the h0 tree, the records' landmark fields
    HIPCHK(top->d_pot.ensure((size_t)V));
    int iters = 0;
    HIPCHK(prep_h0_distances(V, top->d_rowptr.p, adj_out(top), top->d_pot.p, &iters, st));
    top->stats.csr_h0_rounds = iters;
    step_done(3);
    HIPCHK(top->d_sptPar.ensure((size_t)V));
    HIPCHK(top->d_spt.ensure(8 * (size_t)V));
    if (!dir) {
        HIPCHK(prep_tree(V, nadj, hub_segs(top), top->d_rowptr.p, top->d_adj.p, top->d_aloss.p, top->d_pot.p,
                         top->d_sptPar.p, top->d_spt.p, &top->hp->piMax, st));
    } else {
        // kappa0 and the records' field from the out-rows; the tree (a vertex's parent is an
        // in-neighbour, its spt slot an in-row slot) from the in-rows, by their own segments
        HIPCHK(prep_tree(V, nadj, hub_segs(top), top->d_rowptr.p, top->d_adjo.p, nullptr, top->d_pot.p,
                         top->d_sptPar.p, top->d_spt.p, &top->hp->piMax, st, kTreeKappa));
        DevBuf<uint2> iseg;
        DevBuf<uint4> imulti;
        uint32_t ns = 0, nm = 0;
        const int r = make_hub_segs(top->d_rowptrIn.p, H, iseg, imulti, &ns, &nm, st);
        if (r) return r;
        HubSegs hin;
        hin.rows = H;
        hin.seg = iseg.p;
        hin.nseg = ns;
        hin.multi = imulti.p;
        hin.nmulti = nm;
        double pm = 0.0;
        HIPCHK(prep_tree(V, nadj, hin, top->d_rowptrIn.p, top->d_adj.p, top->d_aloss.p, top->d_pot.p,
                         top->d_sptPar.p, top->d_spt.p, &pm, st, kTreeParents));
        // d(v, h0) over the in-rows: the bucket shifts align every source's h0 with it
        // (undirected: d(v, h0) = pi(v))
        DevBuf<double> prev;
        HIPCHK(prev.ensure((size_t)V));
        int it2 = 0;
        HIPCHK(prep_h0_distances(V, top->d_rowptrIn.p, top->d_adj.p, prev.p, &it2, st));
        top->hp->potSrc.resize((size_t)V);
        HIPCHK(hipMemcpyAsync(top->hp->potSrc.data(), prev.p, 8 * (size_t)V, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        double mx = 0.0;
        for (double x : top->hp->potSrc)
            if (std::isfinite(x) && x > mx) mx = x;
        top->hp->srcMax = mx;
    }
    step_done(4);
    // 4) the kappa-sorted relaxation copy (of the out-rows)
    HIPCHK(top->d_adjk.ensure(4 * (size_t)std::max<int64_t>(1, nadj)));
    HIPCHK(top->d_kap.ensure((size_t)std::max<int64_t>(1, nadj)));
    HIPCHK(top->d_ksum.ensure(kKProbes * (size_t)V));
    HIPCHK(top->d_kap0.ensure((size_t)V));
    HIPCHK(launch_kappa_copy(V, nadj, hub_segs(top), top->d_rowptr.p, adj_out(top), top->d_pot.p,
                             top->d_sptPar.p, top->d_adjk.p, top->d_kap.p, top->d_ksum.p,
                             top->d_kap0.p, st));
    top->adjkPlain = true;
    top->adjkFlagged = false;
    top->adjkLeaf = false;
    top->adjkTargets.clear();
    top->leafFor.clear();
    top->rowsSorted = true;
    // the kappa fixpoint's static w - pi per out-row entry (the first target preparation's)
    HIPCHK(top->d_kfKap.ensure((size_t)std::max<int64_t>(1, nadj)));
    HIPCHK(launch_kfix_kap(adj_out(top), top->d_pot.p, nadj, top->d_kfKap.p, st));
    top->kfKapReady = true;
    step_done(5);
    // 5) what the host keeps
    {
        const auto tc = clk::now();
        top->hp->perm.resize((size_t)V);
        top->hp->inv.resize((size_t)V);
        top->hp->pot.resize((size_t)V);
        top->hp->sptPar.resize((size_t)V);
        HIPCHK(hipMemcpyAsync(top->hp->perm.data(), dperm.p, 4 * (size_t)V, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(top->hp->inv.data(), dinv.p, 4 * (size_t)V, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(top->hp->pot.data(), top->d_pot.p, 8 * (size_t)V, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(top->hp->sptPar.data(), top->d_sptPar.p, 4 * (size_t)V, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        copy_ms += ms_since(tc);
        const auto th = clk::now();
        tree_order(*top->hp);
        host_ms += ms_since(th);
    }
    step_done(6);
    MESSAGE("graph preparation: upload %.1f, relabel %.1f, rows %.1f, h0 distances %.1f (%d "
            "rounds), tree %.1f, kappa copy %.1f, host copies %.1f ms",
            top->stats.csr_step_ms[0], top->stats.csr_step_ms[1], top->stats.csr_step_ms[2],
            top->stats.csr_step_ms[3], iters, top->stats.csr_step_ms[4],
            top->stats.csr_step_ms[5], top->stats.csr_step_ms[6]);
    top->stats.csr_host_ms = host_ms;
    top->stats.csr_copy_ms = copy_ms;
    top->csrUploaded = true;
    return 0;
}

DevCSR dev_csr(Topology* top) {
    DevCSR c;
    c.V = top->g.V;
    c.nadj = (int64_t)(top->d_adj.n / 4);
    c.rowptr = top->d_rowptr.p;
    c.rowptr_in = rowptr_in(top);
    c.directed = top->isDirected ? 1 : 0;
    c.adj = top->d_adj.p;
    c.adjk = top->d_adjk.p;
    c.kap = top->d_kap.p;
    c.ksum = reinterpret_cast<const float4*>(top->d_ksum.p);
    c.kap0 = top->d_kap0.p;
    c.spt = top->d_spt.p;
    c.piMax = top->hp->piMax;
    c.aloss = top->d_aloss.p;
    c.vloss = top->d_vloss.p;
    c.selfLat = top->d_selfLat.p;
    c.selfLoss = top->d_selfLoss.p;
    c.rows_sorted = top->rowsSorted ? 1 : 0;
    // marks of the launch's target set; 2: of the effective set, peeled leaf targets dead
    c.tflags = top->adjkFlagged && top->targetSkip ? (top->adjkLeaf ? 2 : 1) : 0;
    return c;
}

int batch_k(Topology* top) { return top->batchK; }  // 2, 4, 8 or 16 (shdtopo_set_option)

// Per-slot u32 scratch after the parent pass' V * K pair list: the merged vertex list (V), then
// 2 bits per vertex (16 per word): the sweep's pending bit and the touched bit (a tail vertex
// whose distance line the batch lowered from +inf: only those lines are reset for the next
// batch), sized as two bitmaps.  Ties live in the pair records' tag words (kTagTie).
int64_t bitmap_words(int64_t n) { return (n + 31) / 32 + 64; }
int64_t ring_entries(Topology* top, int K) {
    const int64_t V = top->g.V;
    // + alignment slack
    return V * (K + 1) + bitmap_words(V) + bitmap_words(V) + 64;
}
int64_t queue_stride(Topology* top, int K) {  // u64 per slot of each near queue / pair list
    const int64_t V = top->g.V;
    return std::max<int64_t>(2 * V, V * K / 2);
}

// The batched SSSP's workspace back to the allocator (a layout change, or a tie-dense topology
// whose builds run only the heap replay: its HBM then holds more replay rows at once).
void release_workspace(Topology* top) {
    if (top->slots <= 0) return;
    top->d_dist.release(); top->d_ring.release(); top->d_rscan.release();
    top->d_prec.release(); top->d_pathbuf.release();
    top->d_qa.release(); top->d_qb.release(); top->d_mask.release(); top->d_hpar.release();
    top->slots = 0;
}

// Per-slot workspace of the batched SSSP: dist [V][K], two K-bit masks per
// vertex, two queues, the per-(vertex, source) parent-pass arrays, the scratch bitmaps.
int ensure_workspace(Topology* top, int nsrc) {
    const int64_t V = top->g.V;
    const int K = batch_k(top);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, top->devId));
    // a short shard runs fewer sources per batch (auto batch_fill), so it can use a slot per
    // source up to the CUs' slots -- sized by sources, not by batches of K (an 8-GPU shard of
    // 1,250 rows got 157 slots for 250 batches of 5: 120 ms instead of 73)
    const int units = top->batchFill > 0 ? (nsrc + top->batchFill - 1) / top->batchFill : nsrc;
    int want = top->slotsOpt > 0 ? top->slotsOpt : prop.multiProcessorCount * kBatchWgPerCu;
    const size_t maskb = 2 * (((size_t)V * (K <= 8 ? 1 : 2) + 255) / 256 * 256);
    const int64_t ringE = ring_entries(top, K);
    const size_t hparN = (size_t)std::min<int64_t>(top->parHubs, 1 << 20) * K;
    // dist (K words/vertex), per-(vertex, source) pair record 16 B, the queues, the u32 scratch,
    // masks, hub hints, path buffer, the row-scan records (16 B per pair of a chunk)
    const int64_t qs = queue_stride(top, K);
    const size_t per_slot = (size_t)V * (8 * (size_t)K + 16 * (size_t)K) + 16 * (size_t)qs +
                            (size_t)ringE * 4 + maskb + 4 * hparN +
                            kPathBufPerSlot * 8 + 16 * (size_t)top->rsChunk * K + 16;
    size_t freeb = 0, totalb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totalb));
    // memory already held by this workspace counts as available
    const size_t held = top->slots > 0 ? (size_t)top->slots * per_slot : 0;
    // engines sharing one device (a multi-engine test configuration) size their workspaces at the
    // same time: each takes its share
    int memcap = (int)std::max<size_t>(
        1, ((freeb + held) * 3 / 5) / (size_t)std::max(1, top->memShareDiv) / per_slot);
    want = std::min(want, memcap);
    want = std::max(1, std::min(want, std::max(1, units)));
    // the batch times of the measured layout (option balance): a launch has at most nsrc batches;
    // allocated here, with the workspace (a fresh allocation right before the launch made the
    // first build's kernel 6-7 ms slower)
    if (top->balance)
        HIPCHK(top->d_btrace.ensure((size_t)std::max<int64_t>(1, std::min<int64_t>(nsrc, V)) * kBTraceWords));
    // hparN follows par_hubs: the kernel indexes the hints at slot * P * K with the current P
    if (top->slots >= want && top->wsK == K && top->wsRing == ringE && top->wsHpar >= hparN &&
        top->wsRsChunk == top->rsChunk) {
        top->stats.workspace_bytes = (int64_t)((size_t)top->slots * per_slot);
        return 0;
    }
    const auto tw0 = std::chrono::steady_clock::now();
    release_workspace(top);  // a layout change: released before re-allocating
    const size_t n = (size_t)want * (size_t)V;
    const size_t pn = n * (size_t)K;  // per-(vertex, source) arrays
    HIPCHK(top->d_dist.ensure(pn));
    HIPCHK(top->d_prec.ensure(pn));
    HIPCHK(top->d_qa.ensure((size_t)want * (size_t)qs));
    HIPCHK(top->d_qb.ensure((size_t)want * (size_t)qs));
    HIPCHK(top->d_ring.ensure((size_t)want * (size_t)ringE));
    HIPCHK(top->d_rscan.ensure((size_t)want * top->rsChunk * K));
    HIPCHK(top->d_pathbuf.ensure((size_t)want * kPathBufPerSlot));
    HIPCHK(top->d_counters.ensure((size_t)want * 4));
    HIPCHK(top->d_mask.ensure((size_t)want * maskb));
    HIPCHK(top->d_hpar.ensure(std::max<size_t>(1, (size_t)want * hparN)));
    HIPCHK(hipMemsetAsync(top->d_mask.p, 0, (size_t)want * maskb, top->stream));
    // every distance starts at +inf and no line is marked touched: a batch resets only the lines
    // it touched (the kernel's init)
    HIPCHK(launch_fill_u64(top->d_dist.p, 0x7FF0000000000000ull, (int64_t)pn, top->stream));
    HIPCHK(hipMemsetAsync(top->d_ring.p, 0, sizeof(uint32_t) * (size_t)want * (size_t)ringE, top->stream));
    // pair records: tag 0 matches no batch (batch tags start at 1); a parent hint of 0 is only
    // a guess the parent pass verifies
    HIPCHK(hipMemsetAsync(top->d_prec.p, 0, sizeof(uint4) * pn, top->stream));
    HIPCHK(hipMemsetAsync(top->d_counters.p, 0, sizeof(uint32_t) * (size_t)want * 4, top->stream));
    HIPCHK(hipStreamSynchronize(top->stream));
    top->slots = want;
    top->wsK = K;
    top->wsHubRows = 0;  // every row +inf
    top->wsRing = ringE;
    top->wsHpar = hparN;
    top->wsRsChunk = top->rsChunk;
    top->stats.slots = want;
    top->stats.workspace_bytes = (int64_t)((size_t)want * per_slot);
    top->stats.workspace_ms = std::chrono::duration<double, std::milli>(
        std::chrono::steady_clock::now() - tw0).count();
    return 0;
}

// Before a batched launch with H LDS hubs: rows [H, wsHubRows) of every slot's dist block may
// still hold hub distances an earlier launch with more hubs copied there (its epilogue); this
// launch treats those vertices as tail vertices, whose lines must start at +inf.
int hub_rows_ready(Topology* top, uint32_t H, hipStream_t st) {
    if (H < top->wsHubRows) {
        const int64_t V = top->g.V, K = top->wsK;
        HIPCHK(launch_fill_u64_strided(top->d_dist.p + (size_t)H * (size_t)K, 0x7FF0000000000000ull,
                                       top->slots, V * K, (int64_t)(top->wsHubRows - H) * K, st));
    }
    top->wsHubRows = H;
    return 0;
}

SlotWs slot_ws(Topology* top) {
    SlotWs w;
    w.slots = top->slots;
    w.V = top->g.V;
    w.dist = top->d_dist.p; w.prec = top->d_prec.p;
    w.qa = top->d_qa.p; w.qb = top->d_qb.p; w.ring = top->d_ring.p;
    w.rscan = top->d_rscan.p;
    w.rs_chunk = top->wsRsChunk;
    w.pathbuf = top->d_pathbuf.p;
    w.counters = top->d_counters.p;
    w.K = top->wsK;
    w.ring_entries = top->wsRing;
    w.q_stride = queue_stride(top, w.K);
    w.mask = top->d_mask.p;
    w.hpar = top->d_hpar.p;
    return w;
}

// Incidence-order CSR of the heap replay (ReplayCSR in topo_device.h).  Row x (relabelled id)
// lists x's igraph_incident edges (type_indexededgelist.c): undirected = out-list (from == x,
// i.e. neighbours <= x) then in-list (neighbours >= x), each by (neighbour, edge id) -> ascending
// original neighbour id; directed (mode OUT) = out-neighbours ascending.  Self loops never relax
// and are dropped; a parallel group becomes one entry with the group's minimum latency (same
// heap history, topo_replay.hip) and the lowest edge id's latency/loss for the hop
// (igraph_get_eid as orc_get_eid).  Built on the GPU (prep_replay_csr) from the parsed edges
// upload_csr keeps in HBM.
// One host pass over the parsed edges (the graph is immutable once loaded), run by the attach-time
// preparation thread or else by the first build that needs it:
//   * meanLat, the mean non-loop latency (the batch kernel's bucket width, default_delta);
//   * replayIntOk: u32 heap keys are exact when every relaxed latency (self loops never relax)
//     is a non-negative integer and no tentative distance du + w <= V x max reaches 2^32 - 1
//     (the unreached marker): then every f64 sum the reference forms is an exact integer.
void edge_scan(Topology* top) {
    if (top->meanLat >= 0) return;
    const HostGraph& g = top->g;
    double s = 0.0, wmax = 0.0, wmin = INFINITY;
    int64_t n = 0;
    bool ints = true;
    for (int64_t e = 0; e < g.E; e++) {
        if (g.eu[(size_t)e] == g.ev[(size_t)e]) continue;
        const double w = g.elat[(size_t)e];
        s += w;
        n++;
        wmin = std::min(wmin, w);
        if (!(w >= 0.0) || w != std::floor(w)) ints = false;
        else wmax = std::max(wmax, w);
    }
    top->replayIntOk = ints && (double)g.V * wmax < 4294967295.0;
    top->minLat = n ? wmin : 0.0;
    top->meanLat = n ? s / (double)n : 1.0;
}

int upload_replay_impl(Topology* top);
int upload_replay(Topology* top) {
    if (top->replayUploaded) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int r = upload_replay_impl(top);
    top->stats.replay_prep_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return r;
}

int upload_replay_impl(Topology* top) {
    const HostGraph& g = top->g;
    const int64_t V = g.V, E = g.E;
    const bool dir = top->isDirected;
    const size_t cap = std::max<size_t>(1, (size_t)(dir ? E : 2 * E));
    edge_scan(top);
    HIPCHK(top->d_rrow.ensure((size_t)V + 1));
    HIPCHK(top->d_rrec.ensure(cap));
    HIPCHK(top->d_rown.ensure(cap));
    HIPCHK(top->d_rhop.ensure(cap));
    int64_t nr = 0;
    HIPCHK(prep_replay_csr(V, E, dir ? 1 : 0, top->d_eu.p, top->d_ev.p, top->d_elat.p,
                           top->d_eloss.p, top->d_inv.p, top->d_pot.p,
                           top->d_rrow.p, top->d_rrec.p, top->d_rown.p, top->d_rhop.p, &nr,
                           top->stream));
    top->rnadj = nr;
    top->replayUploaded = true;
    return 0;
}

ReplayCSR replay_csr(Topology* top) {
    ReplayCSR c;
    c.V = top->g.V;
    c.nadj = top->rnadj;
    c.rowptr = top->d_rrow.p;
    c.rec = top->d_rrec.p;
    c.own = top->d_rown.p;
    // pi = d(h0 -> .) from relabelled vertex 0 (upload_csr; over the out-rows when directed)
    c.landmark = (top->replayLandmark && top->hp && !top->hp->pot.empty()) ? 0 : -1;
    c.intKeys = (top->replayIntOpt && top->replayIntOk) ? 1 : 0;
    c.hop = top->d_rhop.p;
    c.vloss = top->d_vloss.p;
    c.selfLat = top->d_selfLat.p;
    c.selfLoss = top->d_selfLoss.p;
    c.tbits = top->d_tbits.p;
    c.ntargets = top->A;
    return c;
}

// Replay workspace: 32 B x V + the path buffer per slot (one wavefront each).  Slots: 20 per CU
// (C4-int: 16 -> 20 per CU raised the replay's rows/s by 8 %, 21 by 0.5 %), as many as the
// rows need, as the free HBM allows (8 GiB kept back), and balanced: the fewest slots that
// finish the rows in the same number of rounds.
int ensure_replay_ws(Topology* top, int nrows) {
    const size_t V = (size_t)top->g.V;
    const bool ik = top->replayIntOpt && top->replayIntOk;
    const size_t nodeB = ik ? 8 : 16;  // heap node: {u32 key, u32 vertex} or {f64 key, u32 vertex, pad}
    const ReplayLayout lay = replay_layout(ik ? 1 : 0, (uint32_t)V);
    const size_t per_slot = 16 * V + nodeB * lay.nodeCap + (size_t)kMaxHops * 64 * 4 + 64;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, top->devId));
    // wavefronts per CU: replay_wpc (20), or as many as the CU's LDS holds (each its heap's top
    // levels)
    const int lds = (replay_lds_bytes(ik ? 1 : 0) + 255) & ~255;
    const int per_cu = std::max(1, std::min(top->replayWpc, (int)(prop.sharedMemPerMultiprocessor > 0 ? prop.sharedMemPerMultiprocessor : 163840) / lds));
    int want = top->replaySlotsOpt > 0 ? top->replaySlotsOpt : prop.multiProcessorCount * per_cu;
    size_t freeb = 0, totalb = 0;
    HIPCHK(hipMemGetInfo(&freeb, &totalb));
    const size_t held = (size_t)top->rslots * per_slot;
    const size_t keep = (size_t)8 << 30;
    const size_t avail = freeb + held > keep ? freeb + held - keep : 0;
    want = std::min<int64_t>(want, std::max<size_t>(1, std::min(avail, (freeb + held) * 9 / 10) / per_slot));
    want = std::max(1, std::min(want, nrows));
    if (top->replaySlotsOpt <= 0) {
        const int rounds = (nrows + want - 1) / want;
        want = (nrows + rounds - 1) / rounds;
    }
    top->rslotsUse = want;
    if (top->rslots >= want && top->rwsInt == ik) return 0;
    top->d_rvrec.release(); top->d_rnode.release(); top->d_rpath.release();
    top->rslots = 0;
    const size_t n = (size_t)want * V;
    const size_t nn = (size_t)want * lay.nodeCap;
    HIPCHK(top->d_rvrec.ensure(n));
    HIPCHK(top->d_rnode.ensure(ik ? (nn + 1) / 2 : nn));  // uint4 units
    top->rwsInt = ik;
    HIPCHK(top->d_rpath.ensure((size_t)want * kMaxHops * 64));
    top->rslots = want;
    return 0;
}

ReplayWs replay_ws(Topology* top) {
    ReplayWs w;
    w.slots = std::min(top->rslots, top->rslotsUse);
    w.vrec = top->d_rvrec.p;
    w.node = top->d_rnode.p;
    w.pathbuf = top->d_rpath.p;
    const ReplayLayout lay = replay_layout(top->rwsInt ? 1 : 0, (uint32_t)top->g.V);
    w.nodeCap = lay.nodeCap;
    w.stdPos = lay.stdPos;
    w.stdBase = lay.stdBase;
    return w;
}

// target bitmap over V (relabelled ids) for the replay's early exit
int upload_target_bits(Topology* top, const std::vector<uint32_t>& tgt, hipStream_t st) {
    const size_t words = ((size_t)top->g.V + 31) / 32;
    std::vector<uint32_t> tb(words, 0u);
    for (uint32_t t : tgt) tb[t >> 5] |= 1u << (t & 31u);
    HIPCHK(top->d_tbits.ensure(words));
    HIPCHK(hipMemcpyAsync(top->d_tbits.p, tb.data(), 4 * words, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // tb must outlive the async copy
    return 0;
}

// Option "leaf_targets" applies: undirected topologies only (a directed one keeps every target).
bool leaf_targets_on(const Topology* top) { return top->leafTargets && !top->isDirected; }

// The leaf-target records of target set tgt (d_tgt: the same set on the device), the effective
// target bitmap and the peeled vertices' bitmap: one small kernel over the targets, run when the
// set changed.
int ensure_leaf_targets(Topology* top, const std::vector<uint32_t>& tgt, const uint32_t* d_tgt,
                        hipStream_t st) {
    if (top->leafFor == tgt && top->d_tleaf.p) return 0;
    const size_t words = ((size_t)top->g.V + 31) / 32;
    const size_t A = tgt.size();
    std::vector<uint32_t> tb(words, 0u);
    for (uint32_t t : tgt) tb[t >> 5] |= 1u << (t & 31u);
    top->leafFor.clear();
    HIPCHK(top->d_tleaf.ensure(2 * std::max<size_t>(1, A)));
    HIPCHK(top->d_tbitsEff.ensure(words));
    HIPCHK(top->d_dead.ensure(words));
    HIPCHK(top->d_leafCount.ensure(1));
    HIPCHK(hipMemcpyAsync(top->d_tbitsEff.p, tb.data(), 4 * words, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(top->d_dead.p, 0, 4 * words, st));
    HIPCHK(hipMemsetAsync(top->d_leafCount.p, 0, 4, st));
    HIPCHK(launch_leaf_targets(top->d_rowptr.p, top->d_adj.p, top->d_aloss.p, d_tgt, (int)A,
                               top->d_tleaf.p, top->d_tbitsEff.p, top->d_dead.p,
                               top->d_leafCount.p, st));
    uint32_t n = 0;
    HIPCHK(hipMemcpyAsync(&n, top->d_leafCount.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // tb and n must outlive the async copies
    top->leafPeeled = (int64_t)n;
    top->leafFor = tgt;
    return 0;
}

// columns = distinct attached vertices in ascending vertex order.  Caller holds buildMu.
// Returns the setGen the geometry corresponds to; a changed attached set invalidates the table.
uint64_t compute_geometry(Topology* top) {
    std::vector<int32_t> vs;
    uint64_t sg;
    {
        // the attached vertices are those with a host (hostsOn, kept by attach / detach) plus the
        // columns a window adapter keeps (deferredOff): one ordered pass over V counters instead
        // of sorting every host's vertex (C4: 100,000 hosts; 3.9 -> ~1 ms of the first build)
        std::shared_lock<std::shared_mutex> lk(top->ipMu);
        sg = top->setGen.load();
        if (top->geomInit && top->geomGen == top->ipGen) return sg;  // no attach / detach since
        top->geomGen = top->ipGen;
        std::vector<int32_t> def(top->deferredOff.begin(), top->deferredOff.end());
        std::sort(def.begin(), def.end());
        vs.reserve(std::max<size_t>(top->A, 16));
        size_t k = 0;
        const uint32_t* on = top->hostsOn.data();
        for (int32_t v = 0; v < top->g.V; v++) {
            while (k < def.size() && def[k] < v) k++;
            if (on[v] || (k < def.size() && def[k] == v)) vs.push_back(v);
        }
    }
    if (top->geomInit && vs == top->attached) return sg;
    top->geomInit = true;
    top->attached = vs;
    top->A = (int64_t)vs.size();
    top->colOf.assign((size_t)top->g.V, -1);
    for (size_t i = 0; i < vs.size(); i++) top->colOf[(size_t)vs[i]] = (int32_t)i;
    top->colOfShared.reset();
    top->tableValid.store(false);
    // complete-branch materialisation bits are per column pair: a new geometry starts them over
    // (a re-touched pair re-offers a latency >= the running minimum: a no-op, shd-topology.c:501)
    // (complete topologies only: the SSSP branch tracks rows, and A x A bits are 12.5 MB at C4)
    if (top->isComplete) {
        auto pb = std::make_unique<Topology::PairBits>();
        pb->words = (size_t)((top->A * top->A + 63) / 64);
        pb->bits.reset(new std::atomic<uint64_t>[std::max<size_t>(1, pb->words)]);
        for (size_t i = 0; i < std::max<size_t>(1, pb->words); i++) pb->bits[i].store(0, std::memory_order_relaxed);
        top->matPair.store(pb.get(), std::memory_order_release);
        top->matPairs.push_back(std::move(pb));
    }
    return sg;
}

// The shifted distance C of the landmark h0 for every source (undirected: d_s(h0) = pi(s), so
// sh_s = C - pi(s) puts h0 at C): the round-4 rule C = piMax + 2 delta, or, with option h0_phase
// p in [0, 1), the smallest C >= piMax + 2 delta whose phase in its bucket is p (bkt(C) = floor(C
// / delta); every shift stays >= 2 delta).
// the phase h0_shift uses (-1: the round-4 shifts)
double h0_phase(Topology* top, double delta) {
    if (top->h0PhaseSet) return top->h0Phase >= 0.0 && top->h0Phase < 1.0 ? top->h0Phase : -1.0;
    edge_scan(top);
    const double gap = std::min(0.01 * delta, 0.5 * top->minLat);
    return gap > 0.0 && gap < delta ? 1.0 - gap / delta : 0.99;
}

double h0_shift(Topology* top, double delta) {
    const double base = top->hp->to_h0_max() + 2.0 * delta;
    const double ph = h0_phase(top, delta);
    if (ph < 0.0) return base;
    const double x = base / delta;
    double b = std::floor(x - ph) + ph;
    if (b < x) b += 1.0;
    return b * delta;
}

double default_delta(Topology* top) {
    if (top->delta > 0) return top->delta;
    edge_scan(top);
    const double mean = top->meanLat;
    // tuned on C4: with h0 closing its bucket (h0_phase 0.98) and no hub
    // speculation the kernel gains from wide buckets (fewer sweeps and near iterations; the
    // landmark filter keeps the relaxations flat) up to ~0.8 x mean and is flat to ~1.3 x mean;
    // 1.0 x mean (~50 ms) sits in the middle of the plateau
    return std::max(1e-9, 1.0 * mean);
}

// bucket shifts of the sources s[0 .. n) (relabelled ids): sh = C - d(src, h0) >= 2 delta puts
// every source's h0 at C (h0_shift; topo_sssp_batch.hip)
std::vector<double> source_shifts(Topology* top, const uint32_t* s, int64_t n, double delta) {
    const double pmax = top->hp->to_h0_max();  // largest finite d(., h0) (upload_csr)
    const double C = h0_shift(top, delta);
    std::vector<double> sh((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const double p = top->hp->to_h0(s[(size_t)i]);
        sh[(size_t)i] = C - (std::isfinite(p) ? p : pmax);
    }
    return sh;
}

// Seed of the batch kernel's landmark bound for a source with p = d(s, h0) of the graph
// preparation (HostPrep::to_h0) on a V-vertex graph: p (1 + m) rounded up, m = max(1e-9,
// 4 V 2^-53); +inf when p is not finite (no route to h0: no bound), 0 for p = 0 (s = h0).
// Why it is an upper bound of the kernel's final d_j(h0): p is the fixpoint of IEEE adds that
// start at the h0 end, the kernel's value the fixpoint of adds that start at the source end.  For
// the path P that attains p, with n < V hops and u = 2^-53: every partial sum is within (1 +- u)
// per add of the exact one, so d_j(h0) <= fwd(P) <= exact(P) (1 + u)^n <= bwd(P) ((1 + u) /
// (1 - u))^n <= p (1 + 2 n u + O((n u)^2)) <= p (1 + m).  The landmark filter, the target skip, the
// kappa cut and the sweeps' kappa0 test are all proved for any h >= the final d_j(h0)
// (topo_sssp_batch.hip), so the seed may stand in for the tentative value from the first
// expansion on.
double h0_seed_of(double p, int64_t V) {
    if (!(p < INFINITY)) return INFINITY;
    if (!(p > 0.0)) return 0.0;
    const double m = std::max(1e-9, 4.0 * (double)std::max<int64_t>(V, 1) * 0x1p-53);
    return std::nextafter(p * (1.0 + m), INFINITY);
}

// landmark bound seeds of the sources s[0 .. n) (relabelled ids); option h0_seed 0: +inf, the
// kernel then learns d_j(h0) from its own tentative value alone
std::vector<double> source_h0_seeds(Topology* top, const uint32_t* s, int64_t n) {
    std::vector<double> hs((size_t)n, INFINITY);
    if (!top->h0Seed) return hs;
    const int64_t V = (int64_t)top->hp->pot.size();  // (a multi-GPU peer shares hp, not the graph)
    for (int64_t i = 0; i < n; i++)
        hs[(size_t)i] = h0_seed_of(top->hp->to_h0(s[(size_t)i]), V);
    return hs;
}

// LDS plan of a batched launch under the current options (lds_hubs, par_hubs)
SsspLdsPlan batch_lds_plan(Topology* top, int K) {
    return sssp_batch_lds_plan(
        K, top->hubLimit, (uint32_t)std::max<int64_t>(0, std::min<int64_t>(top->parHubs, 1 << 20)),
        top->g.V);
}

void push_min_to_engine(double m) {
    if (worker_updateMinTimeJump && m > 0) worker_updateMinTimeJump(m);
}

const double2* tab_lr(const Topology* top) { return top->extLr ? top->extLr : top->d_lr.p; }
const uint16_t* tab_hops(const Topology* top) { return top->extHops ? top->extHops : top->d_hops.p; }

bool table_current(Topology* top) {
    return top->tableValid.load(std::memory_order_acquire) &&
           top->tableGen.load(std::memory_order_acquire) == top->setGen.load();
}

// The engine of device slot d: slot 0 is the Topology itself, the others are peers holding the
// same graph and columns on their own device (stream, CSR copy, workspaces, table).
Topology* slot_engine(Topology* top, int d) { return d == 0 ? top : top->peers[(size_t)d - 1]; }

// whole-table build on this GPU (for the current attached set)
int ensure_table(Topology* top) {
    if (table_current(top)) return 0;
    const auto tw0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(top->buildMu);
    if (table_current(top)) return 0;
    std::unique_lock<std::shared_mutex> tw(top->tabMu);  // no row copy while the table changes
    const auto tb0 = std::chrono::steady_clock::now();
    // (waiting for the attach-time preparation thread, or another builder)
    top->stats.build_wait_ms = std::chrono::duration<double, std::milli>(tb0 - tw0).count();
    top->stats.attach_prep_ms = top->prepBgMs;
    top->stats.prep_trigger = top->prepStarted.load() ? (top->prepOnLoad ? 2 : 1) : 0;
    for (int i = 0; i < 4; i++) top->stats.attach_prep_step_ms[i] = top->prepStepMs[i];
    for (double& x : top->stats.build_step_ms) x = 0.0;
    top->bstepT = tb0;
    auto bstep = [&](int i) { bstep_mark(top, i); };
    int r = dev_init(top);
    if (r) return r;
    if (getenv("SHDTOPO_TRACE_INIT"))
        fprintf(stderr, "[shdtopo] build: dev_init done at %.2f ms\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count());
    const uint64_t sg = compute_geometry(top);
    bstep(0);
    const int64_t A = top->A;
    reset_build_stats(top);
    int64_t runs0 = top->csrHostRuns;
    for (Topology* p : top->peers) runs0 += p->csrHostRuns;
    top->stats.devices = 1;
    top->stats.exchange_ms = top->stats.exchange_exposed_ms = 0.0;
    top->stats.exchange_bytes = 0;
    if (A > 0 && (top->devicesOpt > 1 || top->forceRccl)) {
        r = build_multi(top);
        if (r) return r;
        if (top->stats.errors) {
            CRITICAL("%lld attached pairs have no path/edge (e.g. a vertex without self loop)",
                     (long long)top->stats.errors);
        }
    } else if (A > 0) {
        HIPCHK(top->d_lr.ensure((size_t)(A * A)));
        bstep(1);
        HIPCHK(top->d_hops.ensure((size_t)(A * A)));
        HIPCHK(top->d_rowmin.ensure((size_t)A));
        r = enqueue_rows(top, 0, A, top->d_lr.p, top->d_hops.p, top->d_rowmin.p, top->stream);
        bstep(4);
        if (r) return r;
        r = collect_row_stats(top);
        bstep(5);
        if (r) return r;
        if (top->stats.errors) {
            CRITICAL("%lld attached pairs have no path/edge (e.g. a vertex without self loop)",
                     (long long)top->stats.errors);
        }
    }
    top->extLr = nullptr;  // the library's own buffers hold the new table
    top->extHops = nullptr;
    int64_t runs1 = top->csrHostRuns;
    for (Topology* p : top->peers) runs1 += p->csrHostRuns;
    top->stats.csr_host_runs = runs1 - runs0;
    top->stats.csr_host_runs_total = runs1;
    top->stats.build_wall_ms = std::chrono::duration<double, std::milli>(
        std::chrono::steady_clock::now() - tb0).count();
    top->spTotalSec += top->stats.build_wall_ms / 1e3;
    top->spCount += (uint64_t)A;
    top->tableGen.store(sg, std::memory_order_release);
    top->tableSerial.fetch_add(1);
    top->tableValid.store(true, std::memory_order_release);
    if (!top->firstTableDone && top->firstAttachSet.load()) {
        top->firstTableDone = true;
        top->stats.first_attach_to_table_ms = std::chrono::duration<double, std::milli>(
            std::chrono::steady_clock::now() - top->firstAttachT).count();
    }
    if (!top->lazy && A > 0) push_min_to_engine(top->eagerMin);
    return 0;
}

// Host snapshot of the current device table: column map + row minima; its rows are copied on
// first use (snap_row).  Published atomically; readers keep the old one alive.
int ensure_snapshot(Topology* top, std::shared_ptr<const HostTable>* out) {
    for (int attempt = 0; attempt < 4; attempt++) {
        int r = ensure_table(top);
        if (r) return r;
        std::shared_ptr<const HostTable> cur = std::atomic_load(&top->snap);
        if (cur && cur->serial == top->tableSerial.load() && table_current(top)) {
            *out = cur;
            return 0;
        }
        std::lock_guard<std::mutex> lk(top->buildMu);
        if (!table_current(top)) continue;  // an attach / detach raced: rebuild first
        cur = std::atomic_load(&top->snap);
        if (cur && cur->serial == top->tableSerial.load()) {
            *out = cur;
            return 0;
        }
        r = dev_init(top);  // this thread's HIP device = the table's
        if (r) return r;
        auto h = std::make_shared<HostTable>();
        h->gen = top->tableGen.load(std::memory_order_acquire);
        h->serial = top->tableSerial.load();
        h->epoch = top->geomGen;
        h->A = top->A;
        if (!top->colOfShared) top->colOfShared = std::make_shared<const std::vector<int32_t>>(top->colOf);
        h->colOf = top->colOfShared;
        const size_t A = (size_t)top->A;
        h->rowmin.resize(A);
        if (A) HIPCHK(hipMemcpy(h->rowmin.data(), top->d_rowmin.p, sizeof(double) * A, hipMemcpyDeviceToHost));
        h->rows.reset(new std::atomic<const double2*>[A ? A : 1]);
        for (size_t i = 0; i < std::max<size_t>(A, 1); i++) h->rows[i].store(nullptr, std::memory_order_relaxed);
        std::shared_ptr<const HostTable> hc = h;
        std::atomic_store(&top->snap, hc);
        *out = hc;
        return 0;
    }
    CRITICAL("the attached set keeps changing while the routing table is built");
    return -5;
}

// The getters' snapshot of `top`: this thread's cached one while it is still the current table
// (no lock, no reference count traffic: Shadow's workers query from many threads at once),
// else refreshed through ensure_snapshot.  The pointer stays valid until this thread's next call.
// A thread keeps its last snapshot alive until it queries again or exits.
struct SnapCache {
    uint64_t uid = 0;
    std::shared_ptr<const HostTable> h;
};
thread_local SnapCache t_snap;

int getter_snapshot(Topology* top, const HostTable** out) {
    SnapCache& c = t_snap;
    if (c.uid == top->uid && c.h && c.h->serial == top->tableSerial.load(std::memory_order_acquire) &&
        table_current(top)) {
        *out = c.h.get();
        return 0;
    }
    std::shared_ptr<const HostTable> h;
    const int r = ensure_snapshot(top, &h);
    if (r) return r;
    c.uid = top->uid;
    c.h = std::move(h);
    *out = c.h.get();
    return 0;
}

// Row c of a snapshot's table ({latency, reliability} per column), copied from the device table
// the first time a query reads it: one 16 A-byte copy (C4: 160 KB) instead of the whole table.
// Copies run in parallel (the library's copy streams, tabMu shared); two threads racing for the same
// row both copy it and the first to publish wins.  Returns 0 (*out set), 1 when the device table
// is no longer the snapshot's (a rebuild ran in between: the caller takes a new snapshot), or a
// negative error.  Rows already copied are read without a lock (acquire load).
int snap_row(Topology* top, const HostTable& h, int64_t c, const double2** out) {
    const double2* p = h.rows[(size_t)c].load(std::memory_order_acquire);
    if (p) {
        *out = p;
        return 0;
    }
    std::shared_lock<std::shared_mutex> lk(top->tabMu);
    if (!top->tableValid.load(std::memory_order_acquire) || top->tableSerial.load() != h.serial)
        return 1;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(top->devId));  // the table's device, for this (worker) thread
    std::unique_ptr<double2[]> buf(new double2[(size_t)std::max<int64_t>(1, h.A)]);
    const hipStream_t cs = top->cstream[std::hash<std::thread::id>{}(std::this_thread::get_id()) %
                                        Topology::kCopyStreams];
    HIPCHK(hipMemcpyAsync(buf.get(), tab_lr(top) + c * h.A, sizeof(double2) * (size_t)h.A,
                          hipMemcpyDeviceToHost, cs));
    HIPCHK(hipStreamSynchronize(cs));
    const double2* expect = nullptr;
    if (h.rows[(size_t)c].compare_exchange_strong(expect, buf.get(), std::memory_order_acq_rel)) {
        *out = buf.get();
        std::lock_guard<std::mutex> g(h.storeMu);
        h.rowStore.push_back(std::move(buf));
    } else {
        *out = expect;  // another thread published this row first
    }
    top->rowsToHost.fetch_add(1, std::memory_order_relaxed);
    top->rowsToHostNs.fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                    std::chrono::steady_clock::now() - t0).count(),
                                std::memory_order_relaxed);
    return 0;
}

// virtualIP[ip] = v (v < 0: not attached) in the getters' lock-free table.  Caller holds ipMu
// exclusively.  The table doubles at half load; the old one stays readable (a reader that loaded
// it sees the state before this write).
void ip_tab_set(Topology* top, uint32_t ip, int32_t v) {
    IpTable* t = top->ipTab.load(std::memory_order_relaxed);
    if (!t || 2 * (t->used + 1) > t->mask + 1) {
        auto n = std::make_unique<IpTable>(t ? 2 * (t->mask + 1) : 1024);
        if (t)
            for (uint64_t i = 0; i <= t->mask; i++) {
                const uint64_t w = t->slot[i].load(std::memory_order_relaxed);
                if (!w) continue;
                n->slot[n->place((uint32_t)(w >> 32))].store(w, std::memory_order_relaxed);
                n->used++;
            }
        t = n.get();
        top->ipTabs.push_back(std::move(n));
        top->ipTab.store(t, std::memory_order_release);
    }
    const uint64_t i = t->place(ip);
    if (t->slot[i].load(std::memory_order_relaxed) == 0) t->used++;
    const uint32_t lo = v < 0 ? IpTable::kTomb : (uint32_t)v + 2u;
    t->slot[i].store(((uint64_t)ip << 32) | lo, std::memory_order_release);
}

// _topology_getConnectedVertexIndex (shd-topology.c:514-531) without the lock
int32_t vertex_of_ip(Topology* top, uint32_t ip) {
    const IpTable* t = top->ipTab.load(std::memory_order_acquire);
    return t ? t->find(ip) : -1;
}

void lazy_store_min(Topology* top, double lat) {
    // shd-topology.c:500-511: if (min == 0 || lat < min) { min = lat; push }
    std::lock_guard<std::mutex> lk(top->minMu);
    if (top->lazyMin == 0 || lat < top->lazyMin) {
        top->lazyMin = lat;
        push_min_to_engine(lat);
    }
}

// Does the reference's cache hold (s, t)?  Only if row s was computed at an epoch when t was
// attached (shd-topology.c:690-744 build the targets from the attached set of that moment).
// Fast path: s materialised after the latest attach interval started covers every vertex
// attached now (the only ones a query can name).
bool lazy_covered(Topology* top, int32_t s, int32_t t) {
    const uint64_t g = top->matGen[(size_t)s].load(std::memory_order_acquire);
    if (g == 0) return false;
    if (g >= top->lastNewEpoch.load(std::memory_order_acquire)) return true;
    std::lock_guard<std::mutex> lk(top->lazyMu);
    std::shared_lock<std::shared_mutex> lk2(top->ipMu);
    auto m = top->matEpochs.find(s);
    auto iv = top->ivals.find(t);
    if (m == top->matEpochs.end() || iv == top->ivals.end()) return false;
    for (uint64_t e : m->second)
        for (const auto& p : iv->second)
            if (p.first <= e && e < p.second) return true;
    return false;
}

// computeSourcePaths(s) now: row s over the current targets enters the cache and its minimum the
// running minimum (shd-topology.c:808-823, :500-511).  e = the attach epoch of the table the row
// is read from (HostTable::epoch): the row covers the vertices attached then -- a vertex attached
// after that table was built is not in it, as if the query had run before that attach.
void lazy_materialise(Topology* top, int32_t s, double rowmin, uint64_t e) {
    {
        std::lock_guard<std::mutex> lk(top->lazyMu);
        auto& v = top->matEpochs[s];  // ascending (a query on an older snapshot may come late)
        auto it = std::lower_bound(v.begin(), v.end(), e);
        if (it == v.end() || *it != e) v.insert(it, e);
        if (v.back() == e) top->matMin[s] = rowmin;
    }
    uint64_t old = top->matGen[(size_t)s].load();
    while (old < e && !top->matGen[(size_t)s].compare_exchange_weak(old, e)) {
    }
    if (rowmin > 0 && !std::isinf(rowmin)) lazy_store_min(top, rowmin);
}

// The minimum of row s over the vertices attached NOW (shd-topology.c:690-744 take the targets
// attached at the moment the row is computed).  The table's row minimum also covers the columns a
// window adapter keeps for vertices that lost their last host (deferredOff, until the flush): while
// such a column exists, row s is read (rowS, or copied now) and those columns are left out
// (ADVICE r04).
double lazy_row_min(Topology* top, const HostTable& h, int32_t s, const double2* rowS) {
    const int64_t cs = h.col(s);
    std::vector<int32_t> gone;
    {
        std::shared_lock<std::shared_mutex> lk(top->ipMu);
        for (int32_t v : top->deferredOff)
            if (top->hostsOn[(size_t)v] == 0) gone.push_back(v);
    }
    if (gone.empty()) return h.rowmin[(size_t)cs];
    if (!rowS && snap_row(top, h, cs, &rowS) != 0) {
        WARNING("row %lld of the routing table could not be read: the running minimum takes the "
                "table's row minimum", (long long)cs);
        return h.rowmin[(size_t)cs];
    }
    std::vector<uint8_t> skip((size_t)h.A, 0);
    for (int32_t v : gone) {
        const int32_t c = h.col(v);
        if (c >= 0 && c < h.A) skip[(size_t)c] = 1;
    }
    double m = INFINITY;
    for (int64_t c = 0; c < h.A; c++) {
        const double x = rowS[c].x;
        if (!skip[(size_t)c] && x >= 0 && x < m) m = x;
    }
    return m;
}

// First-rooted-wins orientation of the SSSP branch (shd-topology.c:894-915):
// (s,d) is answered from row s if the cache holds (s,d) (0), else from row d if it holds (d,s)
// and the graph is undirected (1), else s's row is computed now (2: row s, materialised by the
// caller once it has read the row).
int lazy_orientation(Topology* top, int32_t s, int32_t d) {
    if (lazy_covered(top, s, d)) return 0;
    if (!top->isDirected && lazy_covered(top, d, s)) return 1;
    return 2;
}

// Per-pair first touch of the complete branch (shd-topology.c:894-915 + :835-873): the pair's
// values are symmetric bit for bit, only the running minimum depends on the order.  lat = the
// table's latency of (cs, cd).
void lazy_touch_pair(Topology* top, const HostTable& h, int64_t cs, int64_t cd, double lat) {
    const int64_t A = h.A;
    const size_t b1 = (size_t)(cs * A + cd), b2 = (size_t)(cd * A + cs);
    const Topology::PairBits* pb = top->matPair.load(std::memory_order_acquire);
    if (!pb || pb->words * 64 < (size_t)(A * A)) return;  // geometry moved on (raced)
    bool have = (pb->bits[b1 >> 6].load(std::memory_order_relaxed) >> (b1 & 63)) & 1;
    if (!have && !top->isDirected)
        have = (pb->bits[b2 >> 6].load(std::memory_order_relaxed) >> (b2 & 63)) & 1;
    if (!have) {
        uint64_t old = pb->bits[b1 >> 6].fetch_or(1ull << (b1 & 63));
        if (!((old >> (b1 & 63)) & 1) && lat > 0) lazy_store_min(top, lat);
    }
}

// _topology_getPathEntry (shd-topology.c:876-938) over the prebuilt table.  Called concurrently
// from every worker thread (shd-worker.c:179-203,352-360): the snapshot is immutable, its rows
// are published once, the lazy state is atomics + short locks.
bool get_path_entry(Topology* top, uint32_t srcIP, uint32_t dstIP, double* lat, double* rel) {
    int32_t s = vertex_of_ip(top, srcIP);
    if (s < 0) {
        CRITICAL("invalid vertex %d, source address is not connected to topology", s);
        return false;
    }
    int32_t d = vertex_of_ip(top, dstIP);
    if (d < 0) {
        CRITICAL("invalid vertex %d, destination address is not connected to topology", d);
        return false;
    }
    for (int attempt = 0; attempt < 8; attempt++) {
        const HostTable* h = nullptr;
        if (getter_snapshot(top, &h)) {
            fatal_or_continue(top, "unable to build the routing table");
            return false;
        }
        const int64_t cs = h->col(s), cd = h->col(d);
        if (cs < 0 || cd < 0) {  // detached / re-attached while this call ran
            CRITICAL("address is not connected to the current routing table");
            return false;
        }
        const bool lz = top->lazy;
        const int how = lz && !top->isComplete ? lazy_orientation(top, s, d) : 0;
        const int64_t rr = how == 1 ? cd : cs, cc = how == 1 ? cs : cd;
        const double2* row = nullptr;
        const int rc = snap_row(top, *h, rr, &row);
        if (rc > 0) continue;  // the table was rebuilt meanwhile: a new snapshot
        if (rc < 0) {
            fatal_or_continue(top, "unable to read the routing table");
            return false;
        }
        const double L = row[cc].x, R = row[cc].y;
        if (lz) {
            if (top->isComplete) lazy_touch_pair(top, *h, cs, cd, L);
            else if (how == 2)
                lazy_materialise(top, s, lazy_row_min(top, *h, s, row), h->epoch);
        }
        if (L < 0) {
            // the reference error()s: "unable to find path between node ..." (shd-topology.c:924)
            fatal_or_continue(top, "unable to find path between attached vertices");
            return false;
        }
        if (lat) *lat = L;
        if (rel) *rel = R;
        return true;
    }
    CRITICAL("the routing table keeps changing under a query");
    return false;
}

// _topology_findAttachmentVertex (shd-topology.c:1068-1152) over the candidate index.
// draw(): one random_nextDouble on the host's stream.
template <class Draw>
int32_t find_attachment_vertex(Topology* top, const char* ipHint, const char* geocodeHint,
                               const char* typeHint, Draw&& draw) {
    const AttachIndex& ix = top->aidx;
    const uint32_t requested = ipHint ? string_to_ip(ipHint) : 0xFFFFFFFFu;
    auto lower = [](const char* s) {
        std::string o(s);
        for (auto& c : o) if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
        return o;
    };
    const std::vector<int32_t>* cands = nullptr;
    std::vector<int32_t> exact;
    bool foundExact = false;
    if (ipHint && requested != 0xFFFFFFFFu && requested != 0u) {
        auto it = ix.byIP.find(requested);
        if (it != ix.byIP.end() && !it->second.empty()) {
            foundExact = true;
            cands = &it->second;  // all matches, vertex order (queues cleared at first match)
        }
    }
    static const std::vector<int32_t> kEmpty;
    bool useLPM = false;
    if (!foundExact) {
        auto count_ips = [&](const std::vector<int32_t>& l) {
            for (int32_t v : l) if (ix.usable[(size_t)v]) return true;
            return false;
        };
        const std::vector<int32_t>* tc = &kEmpty;
        const std::vector<int32_t>* ty = &kEmpty;
        const std::vector<int32_t>* co = &kEmpty;
        if (typeHint) {
            auto it = ix.byType.find(lower(typeHint));
            if (it != ix.byType.end()) ty = &it->second;
        }
        if (geocodeHint) {
            auto it = ix.byCode.find(lower(geocodeHint));
            if (it != ix.byCode.end()) co = &it->second;
        }
        if (typeHint && geocodeHint) {
            auto it = ix.byTypeCode.find(lower(typeHint) + '\x01' + lower(geocodeHint));
            if (it != ix.byTypeCode.end()) tc = &it->second;
        }
        if (!tc->empty()) cands = tc;
        else if (!ty->empty()) cands = ty;
        else if (!co->empty()) cands = co;
        else cands = &ix.all;
        useLPM = ipHint && count_ips(*cands);
    }
    if (!cands || cands->empty()) {
        CRITICAL("no attachment candidates (no vertex id contains \"poi\")");
        return -1;
    }
    if (useLPM && !foundExact) {
        uint32_t bestMatch = 0;
        int32_t best = -1;
        for (int32_t v : *cands) {
            uint32_t m = ix.ip[(size_t)v] & requested;
            if (m > bestMatch) { bestMatch = m; best = v; }
        }
        return best;
    }
    double r = draw();
    int indexRange = (int)cands->size() - 1;
    int chosen = (int)round((double)(indexRange * r));
    return (*cands)[(size_t)chosen];
}

// hosts-per-vertex bookkeeping (caller holds ipMu exclusively, ipGen already advanced): a vertex
// gaining its first host opens an attach interval, losing its last closes it; both change the
// table's columns (setGen)
void host_on(Topology* top, int32_t v) {
    if (top->hostsOn[(size_t)v]++ == 0) {
        top->ivals[v].push_back({top->ipGen, UINT64_MAX});
        top->lastNewEpoch.store(top->ipGen);
        top->setGen.fetch_add(1);
    }
}
void host_off(Topology* top, int32_t v) {
    if (--top->hostsOn[(size_t)v] == 0) {
        auto& iv = top->ivals[v];
        if (!iv.empty()) iv.back().second = top->ipGen;
        if (top->windows > 0) {
            // a window adapter may hold packets this vertex emitted or was sent: the column stays
            // until the flush (shdtopo_window_release), the table stays valid
            top->deferredOff.push_back(v);
            return;
        }
        top->setGen.fetch_add(1);
    }
}

// The attach-time preparation (Topology::prepOnAttach): device init + graph preparation in a
// background thread holding buildMu; a build (or any other buildMu holder) that comes first does
// the work itself and the thread then finds nothing left to do.  Complete topologies have no
// batched-SSSP graph to prepare.
void start_graph_prep(Topology* top, bool onLoad) {
    if (top->isComplete) return;
    if (!onLoad && !top->prepOnAttach) return;
    if (top->prepStarted.exchange(true)) return;
    top->prepOnLoad = onLoad;
    top->prepThread = std::thread([top, onLoad]() {
        std::lock_guard<std::mutex> lk(top->buildMu);
        const bool used = top->deviceUsed;
        const auto t0 = std::chrono::steady_clock::now();
        int n = 0;
        if (!top->devInit && (hipGetDeviceCount(&n) != hipSuccess || n <= 0)) {
            (void)hipGetLastError();
            return;  // no GPU here: the first build reports it
        }
        auto tq = t0;
        auto step = [&](int i) {
            const auto t = std::chrono::steady_clock::now();
            top->prepStepMs[i] = std::chrono::duration<double, std::milli>(t - tq).count();
            tq = t;
        };
        int r = dev_init(top);
        step(0);
        if (!r) r = upload_csr(top);
        step(1);
        edge_scan(top);  // mean latency (bucket width) and the replay's integer-key check
        step(2);
        // the batched SSSP's workspace too, sized for a full table (a build with fewer sources
        // uses a part of it; a different batch width re-allocates)
        if (!r) r = ensure_workspace(top, 1 << 30);
        if (!r && top->targetSkip && top->targetResort)
            r = ensure_kprime_scratch(top, nullptr);
        if (!r) r = hipStreamSynchronize(top->stream) == hipSuccess ? 0 : -1;
        step(3);
        top->prepBgRc = r;
        top->prepBgMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        // preparing at topology_new is not a use of the device: the "device" option may still move
        // the topology (set_option re-prepares on the new device)
        if (onLoad) top->deviceUsed = used;
    });
}

// Everything the graph preparation and the SSSP workspace put on the device (a "device" change
// after topology_new's preparation: the next preparation runs on the new device).  Caller holds
// buildMu; no table, attach or build exists yet.
void release_prepared(Topology* top) {
    release_workspace(top);
    for (auto* b : {&top->d_spt, &top->d_sptPar, &top->d_inv, &top->d_rowptr, &top->d_adj,
                    &top->d_adjo, &top->d_rowptrIn, &top->d_adjk})
        b->release();
    for (auto* b : {&top->d_elat, &top->d_eloss, &top->d_aloss, &top->d_vloss, &top->d_selfLat,
                    &top->d_selfLoss, &top->d_pot, &top->d_kfA, &top->d_kfB, &top->d_kfPart,
                    &top->d_kfKap})
        b->release();
    top->kfKapReady = false;
    top->kfFinal = nullptr;
    top->d_eu.release(); top->d_ev.release();
    top->d_kap.release(); top->d_ksum.release(); top->d_kap0.release();
    top->d_hseg.release(); top->d_hmulti.release(); top->d_kfChanged.release();
    top->d_kpKey.release(); top->d_kpIdx.release();
    top->d_kpRec.release(); top->d_kpTmp.release();
    top->d_kpBigPos.release(); top->d_kpBigRow.release(); top->d_kpBigVal.release();
    top->d_kpBigKey.release();
    top->kpBig = -1;
    top->hsegRows = top->hsegN = top->hmultiN = 0;
    top->csrUploaded = top->rowsSorted = false;
    top->adjkPlain = top->adjkFlagged = top->adjkResorted = top->adjkLeaf = false;
    top->adjkTargets.clear();
    top->leafFor.clear();  // the records hold relabelled ids of the released preparation
    top->ordUploaded = false;
    top->ordHp = nullptr;
    top->hp.reset();
}

// shd-topology.c:1154-1166: g_hash_table_replace(virtualIP, ip, vertex)
void do_attach(Topology* top, uint32_t ip, int32_t v, uint64_t* bwDownOut, uint64_t* bwUpOut) {
    if (!top->firstAttachSet.load(std::memory_order_relaxed)) {
        std::unique_lock<std::shared_mutex> lk(top->ipMu);
        if (!top->firstAttachSet.load()) {
            top->firstAttachT = std::chrono::steady_clock::now();
            top->firstAttachSet.store(true);
        }
    }
    start_graph_prep(top, false);
    {
        std::unique_lock<std::shared_mutex> lk(top->ipMu);
        auto it = top->virtualIP.find(ip);
        const int32_t old = it == top->virtualIP.end() ? -1 : it->second;
        top->virtualIP[ip] = v;
        ip_tab_set(top, ip, v);
        top->ipGen++;
        if (old != v) {
            if (old >= 0) host_off(top, old);
            if (v >= 0) host_on(top, v);
        }
    }
    if (v >= 0) {
        if (bwUpOut) *bwUpOut = (uint64_t)top->g.vbwup[(size_t)v];
        if (bwDownOut) *bwDownOut = (uint64_t)top->g.vbwdown[(size_t)v];
    }
}

// shd-topology.c:1190-1197: only the IP mapping goes; cached paths stay
void do_detach(Topology* top, uint32_t ip) {
    std::unique_lock<std::shared_mutex> lk(top->ipMu);
    auto it = top->virtualIP.find(ip);
    if (it == top->virtualIP.end()) return;
    const int32_t v = it->second;
    top->virtualIP.erase(it);
    ip_tab_set(top, ip, -1);
    top->ipGen++;
    if (v >= 0) host_off(top, v);
}

}  // namespace shdtopo

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int shdtopo_version(void) { return 10000; }

Topology* topology_new(const char* graphPath) {
    if (!graphPath) return nullptr;
    Topology* top = new_topology(true);  // the device initialises while the file is parsed
    std::string err;
    MESSAGE("reading graphml topology graph at '%s'...", graphPath);
    const auto t0 = std::chrono::steady_clock::now();
    if (!graphml_load_file(graphPath, top->g, err)) {
        CRITICAL("reading graphml topology '%s' failed: %s", graphPath, err.c_str());
        topology_free(top);
        return nullptr;
    }
    const auto t1 = std::chrono::steady_clock::now();
    Topology* r = finish_new(top);
    if (r && !getenv("SHDTOPO_NO_LOAD_PREP")) start_graph_prep(r, true);
    const auto t2 = std::chrono::steady_clock::now();
    MESSAGE("graphml parsed in %.3f s, checked in %.3f s",
            std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count());
    return r;
}

Topology* shdtopo_new_from_buffer(const char* graphml, size_t len) {
    if (!graphml) return nullptr;
    Topology* top = new_topology(true);
    std::string err;
    if (!graphml_parse(graphml, len, top->g, err)) {
        CRITICAL("parsing graphml buffer failed: %s", err.c_str());
        topology_free(top);
        return nullptr;
    }
    Topology* r = finish_new(top);
    if (r && !getenv("SHDTOPO_NO_LOAD_PREP")) start_graph_prep(r, true);
    return r;
}

Topology* shdtopo_new_synthetic(const ShdSynthParams* p) {
    if (!p) return nullptr;
    Topology* top = new_topology(false);  // a generator (tools): no device until it is used
    SynthParams sp{p->seed, p->n_routers, p->n_poi, p->n_edges, p->integer_latency,
                   p->alpha > 0 ? p->alpha : 1.0 / 1.1, p->directed ? 1 : 0};
    std::string err;
    if (!synth_graph(sp, top->g, err)) {
        CRITICAL("synthetic topology: %s", err.c_str());
        topology_free(top);
        return nullptr;
    }
    return finish_new(top);
}

void topology_free(Topology* top) {
    if (!top) return;
    if (top->initThread.joinable()) top->initThread.join();
    if (top->prepThread.joinable()) top->prepThread.join();
    // _topology_clearCache (shd-topology.c:434-447): the reference reports its Dijkstra total here
    if (top->g.V > 0 && !top->isPeer)
        MESSAGE("path cache cleared, spent %f seconds computing %u shortest paths",
                top->spTotalSec, (unsigned)top->spCount);
    for (Topology* p : top->peers) topology_free(p);
    top->peers.clear();
    monitors_release(top);
    matrices_release(top);
    release_comms(top);
    if (top->devInit) {
        (void)hipStreamSynchronize(top->stream);
        (void)hipEventDestroy(top->ev0);
        (void)hipEventDestroy(top->ev1);
        (void)hipEventDestroy(top->ev2);
        (void)hipEventDestroy(top->ev3);
        (void)hipEventDestroy(top->evr0);
        (void)hipEventDestroy(top->evr1);
        (void)hipEventDestroy(top->evp0);
        (void)hipEventDestroy(top->evp1);
        (void)hipStreamDestroy(top->stream);
        if (top->xstream) (void)hipStreamDestroy(top->xstream);
        for (hipStream_t c : top->cstream)
            if (c) (void)hipStreamDestroy(c);
    }
    delete top;
}

int shdtopo_set_option(Topology* top, const char* key, double value) {
    if (!top || !key) return -1;
    std::string k(key);
    // flags the getters read on worker threads (atomics): no lock, so they never wait for the
    // attach-time preparation or a build
    if (k == "abort_on_error") { top->abortOnError = value != 0; return 0; }
    if (k == "lazy") { top->lazy = value != 0; return 0; }
    // the device-init and attach-time preparation threads and the builders read the rest under
    // buildMu
    std::lock_guard<std::mutex> lk(top->buildMu);
    if (k == "delta") top->delta = value;
    else if (k == "slots") top->slotsOpt = (int)value;
    else if (k == "device") {
        const int d = (int)value;
        if (d < 0) return -1;
        if (d != top->device) {
            // fixed once an attach or a build uses it; before that, topology_new's background
            // init (and preparation) are released and redone on d
            const bool loadPrep = top->prepStarted.load() && top->prepOnLoad;
            if ((top->prepStarted.load() && !loadPrep) || top->firstAttachSet.load() ||
                top->tableValid.load() || top->deviceUsed)
                return -1;
            if (loadPrep) {
                if (top->prepThread.joinable()) top->prepThread.join();  // done: we hold buildMu
                if (top->devInit) (void)hipSetDevice(top->devId);
                (void)hipStreamSynchronize(top->stream);
                release_prepared(top);
            }
            dev_release(top);
            top->device = d;
            if (loadPrep) {
                top->prepStarted.store(false);
                start_graph_prep(top, true);  // waits for buildMu: runs after this call
            }
        }
    }
    else if (k == "prepare_on_attach") top->prepOnAttach = value != 0;
    else if (k == "lds_hubs") top->hubLimit = (int64_t)value;
    else if (k == "par_hubs") top->parHubs = (int64_t)value;
    else if (k == "row_scan_chunk") {
        if (!(value >= 64 && value <= (double)(1 << 20))) return -1;
        top->rsChunk = (uint32_t)value;
    }
    else if (k == "batch") {
        const int b = (int)value;
        if (b != 2 && b != 4 && b != 8 && b != 16) return -1;
        top->batchK = b;
    }
    else if (k == "iter_guard") top->iterGuard = (uint32_t)std::max(1.0, std::min(4e9, value));
    else if (k == "tie_replay") top->tieReplay = value != 0;
    else if (k == "replay_all") top->replayAll = value != 0;
    else if (k == "replay_slots") top->replaySlotsOpt = (int)value;
    else if (k == "replay_wpc") top->replayWpc = std::max(1, std::min(64, (int)value));
    else if (k == "replay_landmark") top->replayLandmark = value != 0;
    else if (k == "replay_int_keys") top->replayIntOpt = value != 0;
    else if (k == "trace_chunk") {
        if (!(value >= 0 && value <= 1e9)) return -1;
        top->traceChunk = (int)value;
    }
    else if (k == "load_walk") {
        if (value != 0 && value != 1) return -1;
        top->loadWalk = (int)value;
    }
    else if (k == "trace_batch") {
        if (value != 0 && value != 1) return -1;
        top->traceBatch = (int)value;
    }
    else if (k == "monitor_index_mb") {
        if (!(value >= 0)) return -1;
        top->monitorIndexMb = value;
    }
    else if (k == "matrix_mb") {
        if (!(value >= 0)) return -1;
        top->matrixMb = value;
    }
    else if (k == "tie_dense") top->tieDenseOpt = value < 0 ? -1 : (value != 0 ? 1 : 0);
    else if (k == "source_order") top->sourceOrder = (int)value;
    else if (k == "batch_order") top->batchOrder = (int)value;
    else if (k == "batch_fill") top->batchFill = (int)value;
    else if (k == "balance") top->balance = (int)value;
    else if (k == "h0_phase") {
        if (!(value < 1.0)) return -1;
        top->h0Phase = value;
        top->h0PhaseSet = true;
    }
    else if (k == "target_skip") top->targetSkip = value != 0;
    else if (k == "target_kappa") top->targetKappa = (int)value;
    else if (k == "target_resort") top->targetResort = value != 0;
    else if (k == "leaf_targets") top->leafTargets = value != 0;
    else if (k == "h0_seed") {
        top->h0Seed = value != 0;
        top->ordUploaded = false;  // the uploaded layout carries the seeds
    }
    else if (k == "exchange") {
        const int m = (int)value;
        if (m < 0 || m > 2) return -1;
        top->xchgMode = m;
        top->tableValid.store(false);
    }
    else if (k == "devices") {
        const int n = (int)value;
        if (n < 1 || n > 64) return -1;
        if (n != top->devicesOpt) top->tableValid.store(false);
        top->devicesOpt = n;
    } else if (k == "rccl") {
        top->forceRccl = value != 0;
        top->tableValid.store(false);
    }
    else return -1;
    return 0;
}

void topology_attach(Topology* top, Address* address, Random* randomSourcePool, char* ipHint,
                     char* geocodeHint, char* typeHint, uint64_t* bwDownOut, uint64_t* bwUpOut) {
    if (!top || !address) return;
    if (!address_toNetworkIP || !random_nextDouble) {
        fatal_or_continue(top, "Shadow symbols address_toNetworkIP/random_nextDouble not found "
                               "(link into shadow or preload libshdtopo_shim.so)");
        return;
    }
    uint32_t ip = address_toNetworkIP(address);
    int32_t v = find_attachment_vertex(top, ipHint, geocodeHint, typeHint,
                                       [&]() { return random_nextDouble(randomSourcePool); });
    do_attach(top, ip, v, bwDownOut, bwUpOut);
}

int32_t shdtopo_attach_ip(Topology* top, uint32_t ip, uint32_t* rngState, const char* ipHint,
                          const char* geocodeHint, const char* typeHint, uint64_t* bwDownOut,
                          uint64_t* bwUpOut) {
    if (!top || !rngState) return -1;
    int32_t v = find_attachment_vertex(top, ipHint, geocodeHint, typeHint,
                                       [&]() { return rand_r_double(rngState); });
    do_attach(top, ip, v, bwDownOut, bwUpOut);
    return v;
}

void topology_detach(Topology* top, Address* address) {
    if (!top || !address || !address_toNetworkIP) return;
    do_detach(top, address_toNetworkIP(address));
}

void shdtopo_detach_ip(Topology* top, uint32_t ip) {
    if (top) do_detach(top, ip);
}

double shdtopo_get_latency_ip(Topology* top, uint32_t srcIP, uint32_t dstIP) {
    double l = 0;
    if (top && get_path_entry(top, srcIP, dstIP, &l, nullptr)) return l;
    return -1.0;
}

double shdtopo_get_reliability_ip(Topology* top, uint32_t srcIP, uint32_t dstIP) {
    double r = 0;
    if (top && get_path_entry(top, srcIP, dstIP, nullptr, &r)) return r;
    return -1.0;
}

double topology_getLatency(Topology* top, Address* srcAddress, Address* dstAddress) {
    if (!top || !srcAddress || !dstAddress || !address_toNetworkIP) return -1.0;
    return shdtopo_get_latency_ip(top, address_toNetworkIP(srcAddress), address_toNetworkIP(dstAddress));
}

double topology_getReliability(Topology* top, Address* srcAddress, Address* dstAddress) {
    if (!top || !srcAddress || !dstAddress || !address_toNetworkIP) return -1.0;
    return shdtopo_get_reliability_ip(top, address_toNetworkIP(srcAddress), address_toNetworkIP(dstAddress));
}

int topology_isRoutable(Topology* top, Address* srcAddress, Address* dstAddress) {
    return topology_getLatency(top, srcAddress, dstAddress) > -1;
}

double topology_getMinimumLatency(Topology* top) {
    if (!top) return -1.0;
    if (ensure_table(top)) return -1.0;
    return top->eagerMin;
}

double shdtopo_get_lazy_minimum_latency(Topology* top) {
    if (!top) return -1.0;
    std::lock_guard<std::mutex> lk(top->minMu);
    return top->lazyMin;
}

int64_t shdtopo_lazy_rows(Topology* top, int32_t* vertex, uint64_t* epoch, double* rowmin,
                          int64_t cap) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->lazyMu);
    int64_t n = 0;
    for (int32_t v = 0; v < top->g.V; v++) {
        const uint64_t e = top->matGen[(size_t)v].load(std::memory_order_acquire);
        if (e == 0) continue;
        if (n < cap) {
            if (vertex) vertex[n] = v;
            if (epoch) epoch[n] = e;
            if (rowmin) {
                auto it = top->matMin.find(v);
                rowmin[n] = it == top->matMin.end() ? -1.0 : it->second;
            }
        }
        n++;
    }
    return n;
}

int64_t shdtopo_num_vertices(Topology* top) { return top ? top->g.V : -1; }
int64_t shdtopo_num_edges(Topology* top) { return top ? top->g.E : -1; }
int shdtopo_is_complete(Topology* top) { return top ? (int)top->isComplete : -1; }
int shdtopo_is_directed(Topology* top) { return top ? (int)top->isDirected : -1; }

int64_t shdtopo_num_attached(Topology* top) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    compute_geometry(top);
    return top->A;
}

int64_t shdtopo_attached_vertices(Topology* top, int32_t* out, int64_t cap) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    compute_geometry(top);
    int64_t n = std::min<int64_t>(cap, top->A);
    for (int64_t i = 0; i < n; i++) out[i] = top->attached[(size_t)i];
    return top->A;
}

int32_t shdtopo_vertex_of_ip(Topology* top, uint32_t ip) { return top ? vertex_of_ip(top, ip) : -1; }

int32_t shdtopo_column_of_ip(Topology* top, uint32_t ip) {
    if (!top) return -1;
    int32_t v = vertex_of_ip(top, ip);
    if (v < 0) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    compute_geometry(top);
    return top->colOf[(size_t)v];
}

void shdtopo_shard_rows(int64_t A, int n, int d, int64_t* r0, int64_t* r1) {
    const int64_t R = n > 0 ? (A + n - 1) / n : 0;
    const int64_t a = std::min(A, (int64_t)d * R), b = std::min(A, a + R);
    if (r0) *r0 = a;
    if (r1) *r1 = b;
}

int shdtopo_build(Topology* top) {
    if (!top) return -1;
    return ensure_table(top);
}

int shdtopo_build_rows(Topology* top, int64_t row0, int64_t row1, void* d_lr, void* d_hops,
                       void* d_rowmin, void* stream) {
    if (!top || !d_lr || !d_hops) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    std::unique_lock<std::shared_mutex> tw(top->tabMu);
    int r = dev_init(top);
    if (r) return r;
    compute_geometry(top);
    if (row0 < 0 || row1 > top->A || row0 > row1) return -2;
    reset_build_stats(top);
    for (double& x : top->stats.build_step_ms) x = 0.0;
    top->bstepT = std::chrono::steady_clock::now();
    const int64_t runs0 = top->csrHostRuns;
    hipStream_t st = stream ? (hipStream_t)stream : top->stream;
    if (top->extLr) {
        // rows written into a table bound by reference (shdtopo_bind_table_ref): the bound table
        // is no longer a finished table, so the getters must not read it until it is bound again
        const char* b0 = (const char*)top->extLr;
        const char* b1 = b0 + sizeof(double2) * (size_t)(top->A * top->A);
        const char* h0 = (const char*)top->extHops;
        const char* h1 = h0 + sizeof(uint16_t) * (size_t)(top->A * top->A);
        const size_t nr = (size_t)((row1 - row0) * top->A);  // d_lr / d_hops: row row0's output
        const char* o0 = (const char*)d_lr;
        const char* o1 = o0 + sizeof(double2) * nr;
        const char* p0 = (const char*)d_hops;
        const char* p1 = p0 + sizeof(uint16_t) * nr;
        if ((o0 < b1 && b0 < o1) || (p0 < h1 && h0 < p1)) {
            top->tableValid.store(false);
            top->extLr = nullptr;
            top->extHops = nullptr;
        }
    }
    const auto tr0 = std::chrono::steady_clock::now();
    r = enqueue_rows(top, row0, row1, (double2*)d_lr, (uint16_t*)d_hops, (double*)d_rowmin, st);
    if (r) return r;
    top->stats.csr_host_runs = top->csrHostRuns - runs0;
    r = collect_row_stats(top);
    top->stats.build_wall_ms = std::chrono::duration<double, std::milli>(
        std::chrono::steady_clock::now() - tr0).count();
    top->spTotalSec += top->stats.build_wall_ms / 1e3;
    top->spCount += (uint64_t)(row1 - row0);
    return r;
}

int shdtopo_bind_table(Topology* top, const void* d_lr, const void* d_hops, double globalMin,
                       void* stream) {
    if (!top || !d_lr || !d_hops) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    std::unique_lock<std::shared_mutex> tw(top->tabMu);
    int r = dev_init(top);
    if (r) return r;
    const uint64_t sg = compute_geometry(top);
    const size_t n = (size_t)(top->A * top->A);
    hipStream_t st = stream ? (hipStream_t)stream : top->stream;
    HIPCHK(top->d_lr.ensure(n));
    HIPCHK(top->d_hops.ensure(n));
    HIPCHK(top->d_rowmin.ensure((size_t)top->A));
    HIPCHK(hipMemcpyAsync(top->d_lr.p, d_lr, sizeof(double2) * n, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(top->d_hops.p, d_hops, sizeof(uint16_t) * n, hipMemcpyDeviceToDevice, st));
    if (top->A) HIPCHK(launch_row_min(top->A, top->A, top->d_lr.p, top->d_rowmin.p, st));
    HIPCHK(hipStreamSynchronize(st));
    top->extLr = nullptr;
    top->extHops = nullptr;
    top->eagerMin = globalMin;
    top->tableGen.store(sg, std::memory_order_release);
    top->tableSerial.fetch_add(1);
    top->tableValid.store(true, std::memory_order_release);
    return 0;
}

int shdtopo_bind_table_ref(Topology* top, const void* d_lr, const void* d_hops, double globalMin,
                           void* stream) {
    if (!top || !d_lr || !d_hops) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    std::unique_lock<std::shared_mutex> tw(top->tabMu);
    int r = dev_init(top);
    if (r) return r;
    const uint64_t sg = compute_geometry(top);
    hipStream_t st = stream ? (hipStream_t)stream : top->stream;
    HIPCHK(top->d_rowmin.ensure((size_t)top->A));
    if (top->A) HIPCHK(launch_row_min(top->A, top->A, (const double2*)d_lr, top->d_rowmin.p, st));
    HIPCHK(hipStreamSynchronize(st));
    top->extLr = (const double2*)d_lr;
    top->extHops = (const uint16_t*)d_hops;
    top->eagerMin = globalMin;
    top->tableGen.store(sg, std::memory_order_release);
    top->tableSerial.fetch_add(1);
    top->tableValid.store(true, std::memory_order_release);
    return 0;
}

int shdtopo_rebuild(Topology* top) {
    if (!top) return -1;
    {
        std::lock_guard<std::mutex> lk(top->buildMu);
        top->tableValid.store(false);
    }
    return ensure_table(top);
}

int shdtopo_table_to_host(Topology* top, double* lat, double* rel, uint16_t* hops) {
    if (!top) return -1;
    for (int attempt = 0; attempt < 4; attempt++) {
        int r = ensure_table(top);
        if (r) return r;
        std::lock_guard<std::mutex> lk(top->buildMu);
        if (!table_current(top)) continue;  // an attach / detach raced: rebuild first
        r = dev_init(top);
        if (r) return r;
        const size_t n = (size_t)(top->A * top->A);
        if (lat || rel) {  // {lat, rel} records split in 64 MB pieces
            const size_t chunk = (size_t)1 << 22;
            std::vector<double2> lr(std::min(n, chunk));
            for (size_t o = 0; o < n; o += chunk) {
                const size_t m = std::min(chunk, n - o);
                HIPCHK(hipMemcpy(lr.data(), tab_lr(top) + o, sizeof(double2) * m, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < m; i++) {
                    if (lat) lat[o + i] = lr[i].x;
                    if (rel) rel[o + i] = lr[i].y;
                }
            }
        }
        if (hops && n) HIPCHK(hipMemcpy(hops, tab_hops(top), sizeof(uint16_t) * n, hipMemcpyDeviceToHost));
        return 0;
    }
    CRITICAL("the attached set keeps changing while the routing table is built");
    return -5;
}

}  // extern "C"

namespace {
// packet_route_kernel over the installed table; caller holds buildMu (no rebuild in between)
int route_locked(Topology* top, const int32_t* d_srcCol, const int32_t* d_dstCol,
                 const uint32_t* d_payload, const uint32_t* d_stateIn, const uint64_t* d_now,
                 int64_t n, uint64_t jumpNs, int clamp, uint64_t* d_time, uint32_t* d_stateOut,
                 uint8_t* d_delivered, hipStream_t st) {
    HIPCHK(hipEventRecord(top->ev2, st));
    HIPCHK(launch_packet_route(n, d_srcCol, d_dstCol, d_payload, d_stateIn, d_now, tab_lr(top),
                               top->A, jumpNs, clamp, d_time, d_stateOut, d_delivered,
                               top->d_stats.p + ST_ROUTE_BAD, st));
    HIPCHK(hipEventRecord(top->ev3, st));
    top->routePending = true;
    return 0;
}
}  // namespace

extern "C" {

int shdtopo_route_batch_device(Topology* top, const int32_t* d_srcCol, const int32_t* d_dstCol,
                               const uint32_t* d_payload, const uint32_t* d_stateIn,
                               const uint64_t* d_now, int64_t n, uint64_t jumpNs, int clamp,
                               uint64_t* d_time, uint32_t* d_stateOut, uint8_t* d_delivered,
                               void* stream) {
    if (!top) return -1;
    int r = ensure_table(top);
    if (r) return r;
    std::lock_guard<std::mutex> lk(top->buildMu);
    hipStream_t st = stream ? (hipStream_t)stream : top->stream;
    return route_locked(top, d_srcCol, d_dstCol, d_payload, d_stateIn, d_now, n, jumpNs, clamp,
                        d_time, d_stateOut, d_delivered, st);
}

}  // extern "C"

namespace {
// worker_schedulePacket (shd-worker.c:332-370) for n packets given by their vertices (-1: the
// address is not attached).  A packet whose vertex is not a column of the current table is not
// routed: delivered 0, time 0, and rngState the sender's state after its draw (the draw was taken
// at emit).  Returns the number of such packets, or a negative error.
int64_t route_vertices(Topology* top, const int32_t* sv, const int32_t* dv, const uint32_t* pay,
                       const uint32_t* sin, const uint64_t* now, size_t n, uint64_t jumpNs,
                       int clampInterHost, TopoPacketOut* out) {
    std::vector<int32_t> sc(n), dc(n);
    std::vector<uint32_t> sout(n);
    std::vector<uint64_t> tim(n);
    std::vector<uint8_t> dl(n);
    int64_t bad = 0;
    // the snapshot and the device table must be the same build: retry if a rebuild intervened
    for (int attempt = 0;; attempt++) {
        std::shared_ptr<const HostTable> h;
        int r = ensure_snapshot(top, &h);
        if (r) return r;
        std::unique_lock<std::mutex> lk(top->buildMu);
        if (!table_current(top) || h->serial != top->tableSerial.load()) {
            if (attempt < 4) continue;
            CRITICAL("the routing table keeps changing under a packet batch");
            return -5;
        }
        // Lazy mode answers every packet as the reference's getReliability/getLatency pair would
        // in emission order (cache orientation, running-minimum pushes): resolved here,
        // sequentially; the kernel reads the chosen row.
        bad = 0;
        for (size_t i = 0; i < n; i++) {
            sc[i] = sv[i] >= 0 && sv[i] < top->g.V ? h->col(sv[i]) : -1;
            dc[i] = dv[i] >= 0 && dv[i] < top->g.V ? h->col(dv[i]) : -1;
            if (sc[i] < 0 || dc[i] < 0 || sc[i] >= h->A || dc[i] >= h->A) {
                sc[i] = dc[i] = -1;  // not routed (the kernel leaves it undelivered)
                bad++;
                continue;
            }
            if (top->lazy) {
                if (top->isComplete) {
                    const double2* row = nullptr;
                    r = snap_row(top, *h, sc[i], &row);
                    if (r) return r < 0 ? r : -5;  // (serial checked above: cannot be stale)
                    lazy_touch_pair(top, *h, sc[i], dc[i], row[dc[i]].x);
                } else {
                    const int how = lazy_orientation(top, sv[i], dv[i]);
                    if (how == 1) std::swap(sc[i], dc[i]);
                    if (how == 2)
                        lazy_materialise(top, sv[i], lazy_row_min(top, *h, sv[i], nullptr),
                                         h->epoch);
                }
            }
        }
        hipStream_t st = top->stream;
        HIPCHK(top->b_src.ensure(n)); HIPCHK(top->b_dst.ensure(n)); HIPCHK(top->b_pay.ensure(n));
        HIPCHK(top->b_sin.ensure(n)); HIPCHK(top->b_sout.ensure(n)); HIPCHK(top->b_now.ensure(n));
        HIPCHK(top->b_time.ensure(n)); HIPCHK(top->b_dl.ensure(n));
        HIPCHK(hipMemcpyAsync(top->b_src.p, sc.data(), 4 * n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(top->b_dst.p, dc.data(), 4 * n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(top->b_pay.p, pay, 4 * n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(top->b_sin.p, sin, 4 * n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(top->b_now.p, now, 8 * n, hipMemcpyHostToDevice, st));
        r = route_locked(top, top->b_src.p, top->b_dst.p, top->b_pay.p, top->b_sin.p,
                         top->b_now.p, (int64_t)n, jumpNs, clampInterHost, top->b_time.p,
                         top->b_sout.p, top->b_dl.p, st);
        if (r) return r;
        HIPCHK(hipMemcpyAsync(tim.data(), top->b_time.p, 8 * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(sout.data(), top->b_sout.p, 4 * n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(dl.data(), top->b_dl.p, n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        break;
    }
    for (size_t i = 0; i < n; i++) {
        out[i].time = tim[i];
        out[i].rngState = sout[i];
        if (sc[i] < 0) {  // not routed: the state after the sender's one draw
            uint32_t s = sin[i];
            (void)glibc_rand_r(&s);
            out[i].rngState = s;
        }
        out[i].delivered = dl[i];
        out[i]._pad[0] = out[i]._pad[1] = out[i]._pad[2] = 0;
    }
    if (bad) WARNING("%lld packets of a batch have an address that is not attached: not routed",
                     (long long)bad);
    return bad;
}
}  // namespace

extern "C" {

int shdtopo_route_batch_device_slot(Topology* top, int slot, const int32_t* d_srcCol,
                                    const int32_t* d_dstCol, const uint32_t* d_payload,
                                    const uint32_t* d_stateIn, const uint64_t* d_now, int64_t n,
                                    uint64_t jumpNs, int clamp, uint64_t* d_time,
                                    uint32_t* d_stateOut, uint8_t* d_delivered, void* stream) {
    if (!top || slot < 0) return -1;
    int r = ensure_table(top);
    if (r) return r;
    std::lock_guard<std::mutex> lk(top->buildMu);
    if (slot > 0 && (top->stats.devices <= slot || slot > (int)top->peers.size())) return -2;
    Topology* T = slot_engine(top, slot);
    int prev = 0;
    HIPCHK(hipGetDevice(&prev));
    HIPCHK(hipSetDevice(T->device % std::max(1, num_devices())));
    hipStream_t st = stream ? (hipStream_t)stream : T->stream;
    r = route_locked(T, d_srcCol, d_dstCol, d_payload, d_stateIn, d_now, n, jumpNs, clamp, d_time,
                     d_stateOut, d_delivered, st);
    HIPCHK(hipSetDevice(prev));
    return r;
}

int topology_routePacketBatch(Topology* top, const TopoPacketIn* in, TopoPacketOut* out, size_t n,
                              uint64_t jumpNs, int clampInterHost) {
    if (!top || (!in && n) || (!out && n)) return -1;
    if (n == 0) return ensure_table(top);
    std::vector<int32_t> sv(n), dv(n);
    std::vector<uint32_t> pay(n), sin(n);
    std::vector<uint64_t> now(n);
    {
        std::shared_lock<std::shared_mutex> lk(top->ipMu);
        for (size_t i = 0; i < n; i++) {
            auto a = top->virtualIP.find(in[i].srcIP);
            auto b = top->virtualIP.find(in[i].dstIP);
            sv[i] = a == top->virtualIP.end() ? -1 : a->second;
            dv[i] = b == top->virtualIP.end() ? -1 : b->second;
            pay[i] = in[i].payloadLength;
            sin[i] = in[i].rngState;
            now[i] = in[i].now;
        }
    }
    const int64_t r = route_vertices(top, sv.data(), dv.data(), pay.data(), sin.data(), now.data(),
                                     n, jumpNs, clampInterHost, out);
    return r < 0 ? (int)r : (int)std::min<int64_t>(r, INT32_MAX);
}

int shdtopo_window_hold(Topology* top, int delta) {
    if (!top) return -1;
    std::unique_lock<std::shared_mutex> lk(top->ipMu);
    top->windows = std::max(0, top->windows + delta);
    return 0;
}

int shdtopo_window_release(Topology* top) {
    if (!top) return -1;
    std::unique_lock<std::shared_mutex> lk(top->ipMu);
    if (top->deferredOff.empty()) return 0;
    top->deferredOff.clear();
    top->ipGen++;  // the columns change: recomputed (and the table rebuilt) on the next query
    top->setGen.fetch_add(1);
    return 0;
}

int shdtopo_route_batch_vertices(Topology* top, const int32_t* srcVertex, const int32_t* dstVertex,
                                 const uint32_t* payloadLength, const uint32_t* rngState,
                                 const uint64_t* now, size_t n, uint64_t jumpNs,
                                 int clampInterHost, TopoPacketOut* out) {
    if (!top || (n && (!srcVertex || !dstVertex || !payloadLength || !rngState || !now || !out)))
        return -1;
    if (n == 0) return ensure_table(top);
    const int64_t r = route_vertices(top, srcVertex, dstVertex, payloadLength, rngState, now, n,
                                     jumpNs, clampInterHost, out);
    return r < 0 ? (int)r : (int)std::min<int64_t>(r, INT32_MAX);
}

int shdtopo_get_stats(Topology* top, ShdStats* out) {
    if (!top || !out) return -1;
    int r = collect_row_stats(top);
    if (r) return r;
    if (top->routePending) {
        HIPCHK(hipEventSynchronize(top->ev3));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, top->ev2, top->ev3));
        top->stats.route_kernel_ms = ms;
        unsigned long long nb = 0;
        HIPCHK(hipMemcpy(&nb, top->d_stats.p + ST_ROUTE_BAD, sizeof nb, hipMemcpyDeviceToHost));
        top->stats.route_bad_packets = (int64_t)nb;
        top->routePending = false;
    }
    top->stats.rows_to_host = top->rowsToHost.load();
    top->stats.rows_to_host_ms = (double)top->rowsToHostNs.load() / 1e6;
    top->stats.dev_inits = top->devInits;
    top->stats.init_bg_ms = top->initBgMs;
    top->stats.path_seconds_total = top->spTotalSec;
    top->stats.paths_computed = (int64_t)top->spCount;
    *out = top->stats;
    return 0;
}

int shdtopo_test_batch_layout(const double* cost, int64_t rows, double fixed, int fill, int slots,
                              int batch, uint32_t* order, uint32_t* starts, int64_t* nbatches) {
    if (!cost || !order || !starts || !nbatches || rows < 1 || rows > (1 << 30)) return -1;
    std::vector<double> c(cost, cost + rows);
    std::vector<uint32_t> ord, st;
    if (!layout_from_costs(c, fixed, fill, slots, batch, ord, st)) return -1;
    std::copy(ord.begin(), ord.end(), order);
    std::copy(st.begin(), st.end(), starts);
    *nbatches = (int64_t)st.size() - 1;
    return 0;
}

double shdtopo_test_h0_seed(double p, int64_t vertices) { return h0_seed_of(p, vertices); }

int shdtopo_test_segsort(const uint32_t* rowptr, int64_t nseg, const float* keys, int64_t n,
                         int reference, float* keys_out, uint32_t* idx_out) {
    if (!rowptr || !keys || !keys_out || !idx_out || nseg < 1 || n < 1 || n > 0x7FFFFFFF ||
        rowptr[0] != 0 || (int64_t)rowptr[nseg] != n)
        return -1;
    for (int64_t i = 0; i < nseg; i++)
        if (rowptr[i + 1] < rowptr[i]) return -1;
    HIPCHK(hipSetDevice(0));
    hipStream_t st = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    DevBuf<uint32_t> rp, iin, iout, bpos, brow, bval;
    DevBuf<unsigned long long> bkey;
    DevBuf<float> kin, kout;
    DevBuf<uint8_t> tmp;
    std::vector<uint32_t> iota, pos, row;  // outlive every copy (synchronised below)
    auto run = [&]() -> int {
        HIPCHK(rp.ensure((size_t)nseg + 1));
        HIPCHK(iout.ensure((size_t)n));
        HIPCHK(kin.ensure((size_t)n));
        HIPCHK(kout.ensure((size_t)n));
        HIPCHK(hipMemcpyAsync(rp.p, rowptr, 4 * ((size_t)nseg + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(kin.p, keys, 4 * (size_t)n, hipMemcpyHostToDevice, st));
        size_t tb = 0;
        if (reference) {
            iota.resize((size_t)n);
            for (int64_t i = 0; i < n; i++) iota[(size_t)i] = (uint32_t)i;
            HIPCHK(iin.ensure((size_t)n));
            HIPCHK(hipMemcpyAsync(iin.p, iota.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st));
            HIPCHK(segsort_reference(rp.p, nseg, n, kin.p, iin.p, kout.p, iout.p, nullptr, &tb, st));
            HIPCHK(tmp.ensure(std::max<size_t>(1, tb)));
            HIPCHK(segsort_reference(rp.p, nseg, n, kin.p, iin.p, kout.p, iout.p, tmp.p, &tb, st));
        } else {
            SegBig big;
            plan_long_rows(rowptr, nseg, pos, row, &big.end_bit);
            const size_t nb = pos.size();
            HIPCHK(bpos.ensure(std::max<size_t>(1, nb)));
            HIPCHK(brow.ensure(std::max<size_t>(1, nb)));
            HIPCHK(bkey.ensure(std::max<size_t>(1, 2 * nb)));
            HIPCHK(bval.ensure(std::max<size_t>(1, 2 * nb)));
            if (nb) {
                HIPCHK(hipMemcpyAsync(bpos.p, pos.data(), 4 * nb, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(brow.p, row.data(), 4 * nb, hipMemcpyHostToDevice, st));
            }
            HIPCHK(segsort_big_tmp_bytes((int64_t)nb, big.end_bit, &tb));
            HIPCHK(tmp.ensure(std::max<size_t>(1, tb)));
            big.pos = bpos.p;
            big.row = brow.p;
            big.nitems = (int64_t)nb;
            big.keys = bkey.p;
            big.vals = bval.p;
            big.tmp = tmp.p;
            big.tmp_bytes = tmp.n;
            HIPCHK(launch_segsort(rp.p, nseg, n, kin.p, kout.p, iout.p, big, st));
        }
        HIPCHK(hipMemcpyAsync(keys_out, kout.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(idx_out, iout.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    };
    const int r = run();
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    return r;
}

int shdtopo_replay_source(Topology* top, int32_t srcv, int full, double* dist, int32_t* parent) {
    if (!top || !dist || !parent) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    if (srcv < 0 || srcv >= top->g.V || top->isComplete) return -2;
    int r = dev_init(top);
    if (r) return r;
    compute_geometry(top);
    const int64_t A = top->A;
    if (A <= 0) return -2;
    r = upload_csr(top);
    if (r) return r;
    r = upload_replay(top);
    if (r) return r;
    r = ensure_replay_ws(top, 1);
    if (r) return r;
    hipStream_t st = top->stream;
    std::vector<uint32_t> tgt((size_t)A);
    for (int64_t i = 0; i < A; i++) tgt[(size_t)i] = (uint32_t)top->hp->inv[(size_t)top->attached[(size_t)i]];
    r = upload_target_bits(top, tgt, st);
    if (r) return r;
    const uint32_t s = (uint32_t)top->hp->inv[(size_t)srcv], row = 0;
    const size_t V = (size_t)top->g.V;
    DevBuf<uint32_t> d_s, d_row, d_tg;
    DevBuf<double2> d_lr;
    DevBuf<uint16_t> d_h;
    DevBuf<double> d_dist;
    DevBuf<int32_t> d_par;
    HIPCHK(d_s.ensure(1)); HIPCHK(d_row.ensure(1)); HIPCHK(d_tg.ensure((size_t)A));
    HIPCHK(d_lr.ensure((size_t)A)); HIPCHK(d_h.ensure((size_t)A));
    HIPCHK(d_dist.ensure(V)); HIPCHK(d_par.ensure(V));
    HIPCHK(hipMemcpy(d_s.p, &s, 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_row.p, &row, 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tg.p, tgt.data(), 4 * (size_t)A, hipMemcpyHostToDevice));
    // its own counters: the last real build's statistics (not read yet) stay intact
    DevBuf<unsigned long long> d_st;
    HIPCHK(d_st.ensure(ST_COUNT));
    HIPCHK(hipMemsetAsync(d_st.p, 0, sizeof(unsigned long long) * ST_COUNT, st));
    HIPCHK(launch_fill_u64(d_st.p + ST_GLOBAL_MIN, 0x7FF0000000000000ull, 1, st));
    HIPCHK(launch_heap_replay(replay_csr(top), replay_ws(top), d_s.p, d_row.p, 1, d_tg.p, (int)A,
                              full, d_lr.p, d_h.p, nullptr, d_st.p, d_dist.p, d_par.p, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<double> hd(V);
    std::vector<int32_t> hp(V);
    HIPCHK(hipMemcpy(hd.data(), d_dist.p, 8 * V, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hp.data(), d_par.p, 4 * V, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < V; i++) {  // relabelled -> original ids
        const size_t o = (size_t)top->hp->perm[i];
        dist[o] = hd[i];
        parent[o] = hp[i] < 0 ? -1 : top->hp->perm[(size_t)hp[i]];
    }
    return 0;
}

int64_t shdtopo_export_csr(Topology* top, int32_t* perm, uint32_t* rowptr, uint32_t* col,
                           double* pot, uint32_t* treeParent) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    if (top->isComplete || top->isDirected) return -2;
    int r = dev_init(top);
    if (r) return r;
    r = upload_csr(top);
    if (r) return r;
    const size_t V = (size_t)top->g.V, nadj = top->d_adj.n / 4;
    if (perm) memcpy(perm, top->hp->perm.data(), 4 * V);
    if (pot) memcpy(pot, top->hp->pot.data(), 8 * V);
    if (treeParent) memcpy(treeParent, top->hp->sptPar.data(), 4 * V);
    if (rowptr) HIPCHK(hipMemcpy(rowptr, top->d_rowptr.p, 4 * (V + 1), hipMemcpyDeviceToHost));
    if (col && nadj) {
        std::vector<uint32_t> rec(4 * nadj);
        HIPCHK(hipMemcpy(rec.data(), top->d_adj.p, 16 * nadj, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < nadj; k++) col[k] = rec[4 * k];
    }
    return (int64_t)nadj;
}

// Test hook: one prepared array by name (include/shd_topology_abi.h).  Host-kept arrays are copied
// from the host, the others from the device after the library's stream has drained (the target
// preparation of the last build is enqueued asynchronously).
int64_t shdtopo_export_prep(Topology* top, const char* name, void* out, int64_t cap_bytes) {
    if (!top || !name) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    if (top->isComplete) return -2;
    int r = dev_init(top);
    if (r) return r;
    r = upload_csr(top);
    if (r) return r;
    HIPCHK(hipStreamSynchronize(top->stream));
    const size_t V = (size_t)top->g.V, nadj = top->d_adj.p ? top->d_adj.n / 4 : 0;
    const size_t words = (V + 31) / 32;
    const bool dir = top->isDirected;
    const bool leaf = top->d_tleaf.p && !top->leafFor.empty();
    const bool tprep = top->adjkFlagged && top->kfFinal;
    const HostPrep& hp = *top->hp;
    const int32_t state[8] = {top->adjkPlain ? 1 : 0, top->adjkFlagged ? 1 : 0,
                              top->adjkResorted ? 1 : 0, top->adjkLeaf ? 1 : 0, kKProbes,
                              kKapInRec ? 1 : 0, (int32_t)kHubSeg, (int32_t)kGroupHubs};
    struct Arr {
        const char* name;
        const void* host;
        const void* dev;
        size_t bytes;
        bool ok;
    };
    const Arr arrs[] = {
        {"perm", hp.perm.data(), nullptr, 4 * V, true},
        {"inv", hp.inv.data(), nullptr, 4 * V, true},
        {"rowptr", nullptr, top->d_rowptr.p, 4 * (V + 1), true},
        {"adj", nullptr, top->d_adj.p, 16 * nadj, true},
        {"aloss", nullptr, top->d_aloss.p, 8 * nadj, true},
        {"vloss", nullptr, top->d_vloss.p, 8 * V, true},
        {"self_lat", nullptr, top->d_selfLat.p, 8 * V, true},
        {"self_loss", nullptr, top->d_selfLoss.p, 8 * V, true},
        {"pot", hp.pot.data(), nullptr, 8 * V, true},
        {"pi_max", &hp.piMax, nullptr, 8, true},
        {"spt_parent", nullptr, top->d_sptPar.p, 4 * V, true},
        {"spt", nullptr, top->d_spt.p, 32 * V, true},
        {"adjk", nullptr, top->d_adjk.p, 16 * nadj, true},
        {"kap", nullptr, top->d_kap.p, 4 * nadj, true},
        {"ksum", nullptr, top->d_ksum.p, 4 * (size_t)kKProbes * V, true},
        {"kap0", nullptr, top->d_kap0.p, 4 * V, true},
        {"kf_kap", nullptr, top->d_kfKap.p, 8 * nadj, top->kfKapReady},
        {"hub_seg", nullptr, top->d_hseg.p, sizeof(uint2) * (size_t)top->hsegN, true},
        {"hub_multi", nullptr, top->d_hmulti.p, sizeof(uint4) * (size_t)top->hmultiN, true},
        {"rowptr_in", nullptr, top->d_rowptrIn.p, 4 * (V + 1), dir},
        {"adj_out", nullptr, top->d_adjo.p, 16 * nadj, dir},
        {"pot_src", hp.potSrc.data(), nullptr, 8 * V, dir && hp.potSrc.size() == V},
        {"tbits", nullptr, top->d_tbits.p, 4 * words, top->adjkFlagged && top->d_tbits.p},
        {"tbits_eff", nullptr, top->d_tbitsEff.p, 4 * words, leaf},
        {"dead", nullptr, top->d_dead.p, 4 * words, leaf},
        {"tleaf", nullptr, top->d_tleaf.p, 32 * top->leafFor.size(), leaf},
        {"kfix", nullptr, top->kfFinal, 16 * V, tprep},
        {"state", state, nullptr, sizeof state, true},
    };
    for (const Arr& a : arrs) {
        if (strcmp(a.name, name) != 0) continue;
        if (!a.ok) return -2;
        if (!out) return (int64_t)a.bytes;
        if (cap_bytes < (int64_t)a.bytes) return -3;
        if (a.bytes == 0) return 0;
        if (a.host) memcpy(out, a.host, a.bytes);
        else if (a.dev) HIPCHK(hipMemcpy(out, a.dev, a.bytes, hipMemcpyDeviceToHost));
        else return -2;
        return (int64_t)a.bytes;
    }
    return -1;
}

int shdtopo_export_graph(Topology* top, int32_t* eu, int32_t* ev, double* elat, double* eloss,
                         double* vloss) {
    if (!top) return -1;
    const HostGraph& g = top->g;
    const size_t E = (size_t)g.E, V = (size_t)g.V;
    if (eu) memcpy(eu, g.eu.data(), 4 * E);
    if (ev) memcpy(ev, g.ev.data(), 4 * E);
    if (elat) memcpy(elat, g.elat.data(), 8 * E);
    if (eloss) memcpy(eloss, g.eloss.data(), 8 * E);
    if (vloss) memcpy(vloss, g.vloss.data(), 8 * V);
    return 0;
}

int shdtopo_write_graphml(Topology* top, const char* path) {
    if (!top || !path) return -1;
    return graphml_write_file(top->g, path) ? 0 : -1;
}

int shdtopo_synth_packets(Topology* top, uint64_t seed, int64_t n_hosts, int64_t n_packets,
                          uint64_t t0, uint64_t jump, int32_t* srcCol, int32_t* dstCol,
                          uint32_t* payload, uint32_t* stateIn, uint64_t* now, uint32_t* srcIP,
                          uint32_t* dstIP) {
    if (!top || n_hosts < 2) return -1;
    // seed chain: master Random(seed) -> slave seed = rand_r(master) ->
    // per-host nodeSeed = rand_r(slave) (shd-master.c:65,134; shd-create-node.c:216)
    uint32_t master = (uint32_t)seed;
    uint32_t slave = (uint32_t)glibc_rand_r(&master);
    std::vector<uint32_t> hostState((size_t)n_hosts), hostIP((size_t)n_hosts);
    std::vector<int32_t> hostVertex((size_t)n_hosts);
    std::vector<int> role((size_t)n_hosts);
    static const char* kRole[] = {"client", "relay", "server"};
    std::vector<int64_t> relays, servers;
    for (int64_t h = 0; h < n_hosts; h++) {
        int64_t m = h % 100;
        role[(size_t)h] = m < 94 ? 0 : (m < 99 ? 1 : 2);
        if (role[(size_t)h] == 1) relays.push_back(h);
        if (role[(size_t)h] == 2) servers.push_back(h);
        hostState[(size_t)h] = (uint32_t)glibc_rand_r(&slave);
        hostIP[(size_t)h] = htonl(0x0B000001u + (uint32_t)h);
        // the first hosts are pinned one per poi by an exact ipHint (shd-topology.c:1087-1100,
        // no random draw), so every poi is attached (A = n_poi); the rest attach by type hint
        const char* iphint = nullptr;
        std::string hs;
        if (h < (int64_t)top->aidx.all.size() && top->aidx.usable[(size_t)top->aidx.all[(size_t)h]]) {
            hs = top->g.vip[(size_t)top->aidx.all[(size_t)h]];
            iphint = hs.c_str();
        }
        hostVertex[(size_t)h] = shdtopo_attach_ip(top, hostIP[(size_t)h], &hostState[(size_t)h],
                                                  iphint, nullptr, kRole[role[(size_t)h]],
                                                  nullptr, nullptr);
        if (hostVertex[(size_t)h] < 0) return -2;
    }
    if (relays.empty()) relays.push_back(0);
    if (servers.empty()) servers = relays;
    if (n_packets <= 0) return 0;  // the attach phase only
    // the table's columns (ascending attached vertex) from the attach table itself: the harness
    // takes no build lock, so any wait for the attach-time preparation shows in the build
    std::vector<int32_t> cols;
    {
        // as compute_geometry: the attached vertices plus the columns a window adapter keeps
        std::shared_lock<std::shared_mutex> lk(top->ipMu);
        cols.reserve(top->virtualIP.size() + top->deferredOff.size());
        for (auto& kv : top->virtualIP)
            if (kv.second >= 0) cols.push_back(kv.second);
        cols.insert(cols.end(), top->deferredOff.begin(), top->deferredOff.end());
    }
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    auto colOf = [&](int32_t v) {
        return (int32_t)(std::lower_bound(cols.begin(), cols.end(), v) - cols.begin());
    };
    SplitMix rng(seed ^ 0x5eed5eed5eedull);
    for (int64_t k = 0; k < n_packets; k++) {
        int64_t s = (int64_t)rng.below((uint64_t)n_hosts);
        int64_t d;
        do {
            int rl = role[(size_t)s];
            if (rl == 0 || rl == 2) d = relays[(size_t)rng.below(relays.size())];
            else d = (rng.below(2) == 0) ? relays[(size_t)rng.below(relays.size())]
                                         : servers[(size_t)rng.below(servers.size())];
        } while (d == s && n_hosts > 1 && relays.size() + servers.size() > 1);
        srcCol[k] = colOf(hostVertex[(size_t)s]);
        dstCol[k] = colOf(hostVertex[(size_t)d]);
        payload[k] = rng.uniform() < 0.8 ? 1448u : 0u;
        stateIn[k] = hostState[(size_t)s];
        (void)glibc_rand_r(&hostState[(size_t)s]);  // the route's draw advances the host stream
        now[k] = t0 + (jump ? rng.below(jump) : 0);
        if (srcIP) srcIP[k] = hostIP[(size_t)s];
        if (dstIP) dstIP[k] = hostIP[(size_t)d];
    }
    return 0;
}

}  // extern "C"
