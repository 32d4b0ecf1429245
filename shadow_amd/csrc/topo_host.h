// topo_host.h -- what the host units of libshdtopo (topo_core.cpp, topo_build.cpp, topo_flows.cpp,
// topo_monitor_host.cpp, topo_matrix_host.cpp, topo_whatif.cpp) share: logging, DevBuf, DevEvents, struct _Topology, the
// core functions the table build, the flow analysis and the what-if family call and the flow
// analysis' own shared parts.  Included by the .cpp units only.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <deque>
#include <functional>
#include <thread>

#include "../../include/shd_topology_abi.h"
#include "topo_internal.h"

namespace shdtopo {

// GLib log levels (G_LOG_LEVEL_CRITICAL / WARNING / MESSAGE / INFO)
constexpr int kLogCritical = 1 << 3, kLogWarning = 1 << 4, kLogMessage = 1 << 5, kLogInfo = 1 << 6;

// The reference's critical() / warning() / message() (shd-logging.h:24-59): inside Shadow the
// message goes through logging_log, which filters by the configured level and adds the run's
// prefix; standalone it goes to stderr, filtered by SHDTOPO_LOG (topo_core.cpp).
void shd_log(int glevel, const char* file, const char* func, int line, const char* fmt, ...);
#define CRITICAL(...) shd_log(kLogCritical, __FILE__, __FUNCTION__, __LINE__, __VA_ARGS__)
#define WARNING(...) shd_log(kLogWarning, __FILE__, __FUNCTION__, __LINE__, __VA_ARGS__)
#define MESSAGE(...) shd_log(kLogMessage, __FILE__, __FUNCTION__, __LINE__, __VA_ARGS__)
#define INFO(...) shd_log(kLogInfo, __FILE__, __FUNCTION__, __LINE__, __VA_ARGS__)

#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            CRITICAL("HIP error %s at %s:%d (%s)", hipGetErrorString(_e), __FILE__, __LINE__, \
                     #expr);                                                                \
            return -100 - (int)_e;                                                          \
        }                                                                                   \
    } while (0)
// a step that returns 0 or its error
#define CHK(expr)              \
    do {                       \
        const int _r = (expr); \
        if (_r) return _r;     \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&p, sizeof(T) * (count ? count : 1));
        if (e == hipSuccess) n = count;
        else p = nullptr;
        return e;
    }
};

// N events of one call's own, destroyed with it (hidden: the library exports no instantiation)
template <int N>
struct __attribute__((visibility("hidden"))) DevEvents {
    hipEvent_t e[N] = {};
    int create() {
        for (hipEvent_t& x : e) HIPCHK(hipEventCreate(&x));
        return 0;
    }
    ~DevEvents() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

// wall-clock milliseconds since t
inline double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// Open-addressing IP -> vertex table read by the getters without a lock (Shadow calls them from
// every worker thread, shd-worker.c:179-203; the reference takes virtualIPLock per lookup,
// shd-topology.c:514-531).  A slot holds (ip << 32) | (vertex + 2); 0 = empty, low word kTomb =
// detached.  An IP keeps its slot for the table's lifetime, so a lookup stops at its key or at an
// empty slot.  Writers (attach / detach) are serialised by Topology::ipMu.
struct IpTable {
    static constexpr uint32_t kTomb = 0xFFFFFFFFu;
    uint64_t mask = 0;
    size_t used = 0;
    std::unique_ptr<std::atomic<uint64_t>[]> slot;
    explicit IpTable(uint64_t cap) : mask(cap - 1), slot(new std::atomic<uint64_t>[cap]) {
        for (uint64_t i = 0; i < cap; i++) slot[i].store(0, std::memory_order_relaxed);
    }
    uint64_t home(uint32_t ip) const { return ((uint64_t)ip * 0x9E3779B97F4A7C15ull >> 17) & mask; }
    int32_t find(uint32_t ip) const {
        for (uint64_t i = home(ip);; i = (i + 1) & mask) {
            const uint64_t w = slot[i].load(std::memory_order_acquire);
            if (w == 0) return -1;
            if ((uint32_t)(w >> 32) == ip) {
                const uint32_t lo = (uint32_t)w;
                return lo == kTomb ? -1 : (int32_t)(lo - 2);
            }
        }
    }
    // writer: the slot of ip (existing, else the first empty one)
    uint64_t place(uint32_t ip) const {
        for (uint64_t i = home(ip);; i = (i + 1) & mask) {
            const uint64_t w = slot[i].load(std::memory_order_relaxed);
            if (w == 0 || (uint32_t)(w >> 32) == ip) return i;
        }
    }
};

uint64_t next_topology_uid();
// link monitors (shdtopo_monitor_*, topo_monitor_host.cpp): ids are unique in the process, so
// another topology's id is never found in this one's list
struct LinkMonitor;
// traffic matrices (shdtopo_matrix_*, topo_matrix_host.cpp): ids likewise
struct TrafficMatrix;

}  // namespace shdtopo
using namespace shdtopo;

struct _Topology {
    // the parsed graph; the peer engines of a multi-GPU build share the owner's (read-only)
    std::shared_ptr<HostGraph> gp = std::make_shared<HostGraph>();
    HostGraph& g = *gp;
    _Topology() = default;
    explicit _Topology(std::shared_ptr<HostGraph> shared) : gp(std::move(shared)), g(*gp) {}

    bool isComplete = false;
    bool isDirected = false;
    bool isPeer = false;  // a peer engine of a multi-GPU build (make_peer), not a caller's topology
    bool hasMultiEdges = false;
    // link failure what-if (shdtopo_derive_without): per edge its id in the root topology (empty:
    // the identity, a root topology), the vertices failed on the way here (empty: none; they are
    // isolated, exempt from the connectivity check and no attachment candidates), and whether
    // the derivation already checked the connectivity of the rest
    std::vector<int32_t> edgeOrigin;
    std::vector<uint8_t> failedVertex;
    bool preChecked = false;
    int64_t rootE = -1;  // a derived topology: the root's edge count, inherited (-1: a root, g.E)
    ShdDiffStats diffStats{};  // table diff (shdtopo_table_diff, topo_diff.hip): first argument's
    ShdImpactStats impactStats{};  // flow impact (shdtopo_flow_impact, topo_impact.hip): likewise
    ShdShiftStats shiftStats{};    // load shift (shdtopo_load_shift, topo_shift.hip): likewise
    // route schedule (shdtopo_route_schedule*, topo_schedule.hip): tops[0]'s -- the last call's
    // statistics, the call's epoch counters (u64 [16][3]) and the host variants' epoch bytes
    ShdScheduleStats scheduleStats{};
    DevBuf<unsigned long long> d_schedCnt;
    DevBuf<uint8_t> b_ep;

    // options ("abort_on_error" and "lazy" are read by getters on worker threads without a lock)
    std::atomic<bool> abortOnError{true};
    std::atomic<bool> lazy{true};
    double delta = 0.0;  // 0 = auto
    int slotsOpt = 0;
    int device = 0;
    int64_t hubLimit = -1;  // LDS-cached hub distances (-1 = fill the LDS)
    int64_t parHubs = 2048; // hubs whose parent is hinted during the SSSP (0 = always scan)
    uint32_t rsChunk = kRowScanCap;  // pairs per parent-pass row-scan chunk
    int batchK = 8;         // sources per SSSP workgroup (sssp_batch_kernel<K>, K in {2,4,8,16})
    uint32_t iterGuard = 4000000u;  // near iterations per batch before the kernel gives up
                                    // (option "iter_guard": a test hook for the -4 error path)

    // attach state (shd-topology.c:20-24 virtualIP)
    std::shared_mutex ipMu;
    std::unordered_map<uint32_t, int32_t> virtualIP;
    AttachIndex aidx;
    // the getters' lock-free view of virtualIP (IpTable): written under ipMu (exclusive) next to
    // the map, read with acquire loads and no lock; superseded tables stay allocated until free
    std::atomic<IpTable*> ipTab{nullptr};
    std::vector<std::unique_ptr<IpTable>> ipTabs;
    const uint64_t uid = next_topology_uid();  // identifies this topology to thread-local caches

    // table geometry
    std::mutex buildMu;
    // writers of the device table (builds, binds) hold it exclusively inside buildMu; the getters'
    // row copies (snap_row) hold it shared, so they run in parallel and never see a half-built table
    std::shared_mutex tabMu;
    std::atomic<bool> tableValid{false};
    std::vector<int32_t> attached;  // columns: distinct attached vertices, ascending
    std::vector<int32_t> colOf;     // vertex -> column
    std::shared_ptr<const std::vector<int32_t>> colOfShared;  // colOf for the snapshots (lazily
                                                              // made, reset with the geometry)
    int64_t A = 0;

    // device state
    bool devInit = false;
    // any entry point asked this engine's device for work (every one goes through dev_init): the
    // "device" option is fixed from then on (buffers, tables and matrices live on that device)
    bool deviceUsed = false;
    int devId = 0;               // the device dev_init bound (every later entry re-binds it)
    int64_t devInits = 0;        // dev_init runs (a "device" change before the first attach
                                 // re-initialises on the new device)
    // Device init at topology_new (shd-topology.c:1237): a background thread holding buildMu
    // initialises the default device (SHDTOPO_DEVICE, else 0) while the GraphML is parsed, so the
    // first attach and the first build no longer pay the HIP context, queues and code objects.
    std::thread initThread;
    double initBgMs = 0.0;       // its wall time
    // Preparation at the first attach (option "prepare_on_attach", default on): a background
    // thread initialises the device and prepares the graph (upload_csr) under buildMu while the
    // host attaches its hosts, so the first table build -- whose lock waits for the thread --
    // no longer pays them.  The device option must be set before the first attach.
    bool prepOnAttach = true;
    // Preparation at topology_new: a non-complete topology loaded from
    // GraphML starts the same thread right after the parse, so the attach phase and everything
    // Shadow does before it hide it (C4: ~50 ms); a later "device" change re-prepares there.
    // SHDTOPO_NO_LOAD_PREP=1 leaves it to the first attach.
    bool prepOnLoad = false;  // the running / finished preparation was started by topology_new
    std::atomic<bool> prepStarted{false};
    std::thread prepThread;
    double prepBgMs = 0.0;       // the thread's wall time
    double prepStepMs[4] = {0, 0, 0, 0};  // of which device init, graph preparation, edge scan,
                                          // SSSP workspace
    // wall clock of the first attach, and whether the first table since then was installed
    // (ShdStats.first_attach_to_table_ms)
    std::chrono::steady_clock::time_point firstAttachT;
    std::atomic<bool> firstAttachSet{false};
    bool firstTableDone = false;
    int prepBgRc = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    bool csrUploaded = false;
    bool rowsSorted = false;
    // host side of the graph preparation (upload_csr): shared with the peer engines of a
    // multi-GPU build, which copy the device CSR from this engine instead of preparing it again
    std::shared_ptr<HostPrep> hp;
    int64_t csrHostRuns = 0;    // host-side preparations (peers that copied count none)
    // per vertex, 32 B: {parent, slot of (v -> parent) in v's row, f64 latency, f64 loss, pad}
    DevBuf<uint32_t> d_spt;
    DevBuf<uint32_t> d_sptPar;  // per vertex: h0-tree parent
    // the parsed edge arrays (document order) and old -> new ids, kept in HBM after the graph
    // preparation: the heap replay's CSR is built from them (prep_replay_csr)
    DevBuf<int32_t> d_eu, d_ev;
    DevBuf<double> d_elat, d_eloss;
    DevBuf<uint32_t> d_inv;
    int wsK = 0;                // batch width the workspace was laid out for
    uint32_t wsHubRows = 0;     // rows [0, wsHubRows) of every slot's dist block may hold a
                                // launch's hub distances (the epilogue copies them there): a
                                // launch with fewer LDS hubs refills [H, wsHubRows) with +inf
    int64_t wsRing = 0;
    size_t wsHpar = 0;          // hub-hint entries per slot the workspace was sized for
    uint32_t wsRsChunk = 0;     // row-scan chunk the workspace was sized for
    DevBuf<uint32_t> d_rowptr, d_adj;
    // directed topologies: d_rowptr / d_adjo are the out-rows (relaxation, kappa copy, target
    // fixpoint), d_rowptrIn / d_adj / d_aloss the in-rows (parent pass); undirected ones use
    // d_rowptr / d_adj for both (d_adjo, d_rowptrIn empty) -- adj_out(), rowptr_in()
    DevBuf<uint32_t> d_adjo, d_rowptrIn;
    DevBuf<uint32_t> d_adjk;  // rows re-sorted by kappa = w - pi(col) (batch relaxation copy)
    DevBuf<float> d_kap, d_ksum, d_kap0;  // kappa of d_adjk (f32, rounded down), per-vertex probes
    double meanLat = -1.0;
    double minLat = 0.0;  // smallest non-loop edge latency (edge_scan): the landmark's bucket gap
    uint64_t ipGen = 1, geomGen = 0;  // attach/detach generation; compute_geometry's copy  // mean non-loop edge latency (default delta), computed once
    DevBuf<double> d_aloss, d_vloss, d_selfLat, d_selfLoss;
    DevBuf<unsigned long long> d_dist, d_qa, d_qb;
    DevBuf<uint32_t> d_ring;
    DevBuf<uint4> d_prec;  // per (vertex, source) pair records of the parent pass
    DevBuf<double> d_pathbuf;
    DevBuf<uint32_t> d_counters;
    DevBuf<uint4> d_rscan;  // parent pass row-scan records, rsChunk x K per slot
    int slots = 0;
    DevBuf<double2> d_lr;
    DevBuf<uint16_t> d_hops;
    // a table installed in place (shdtopo_bind_table_ref): caller-owned HBM read instead of d_lr /
    // d_hops until the next build or bind
    const double2* extLr = nullptr;
    const uint16_t* extHops = nullptr;
    DevBuf<double> d_rowmin;
    DevBuf<double> d_elatAA, d_elossAA, d_vlossA;
    std::vector<int32_t> aaCols;  // the columns the resident A x A edge matrices were built for
    DevBuf<uint32_t> d_sources, d_targets;
    DevBuf<double> d_srcsh;
    DevBuf<double> d_h0seed;  // per layout position: the landmark bound's seed (source_h0_seeds)
    DevBuf<uint8_t> d_mask;
    DevBuf<uint32_t> d_hpar;
    DevBuf<unsigned long long> d_stats;
    // host-batch staging
    DevBuf<int32_t> b_src, b_dst;
    DevBuf<uint32_t> b_pay, b_sin, b_sout;
    DevBuf<uint64_t> b_now, b_time;
    DevBuf<uint8_t> b_dl;

    // exact heap replay (topo_replay.hip): igraph's pop order for rows whose target chains cross
    // a d-tied parent, and every row of a directed topology
    bool tieReplay = true;    // option "tie_replay" (0: report ambiguous pairs only)
    bool replayAll = false;   // option "replay_all" (test hook: every row through the replay)
    // option "tie_dense": -1 auto, 0 never, 1 always.  A tie-dense topology (integer latencies:
    // C4-int replays every row) skips the batch kernel, whose rows the replay would recompute
    // anyway; auto turns it on after a build of >= 64 rows that replayed >= 90 % of them, or
    // before the first batched build of an integer-latency topology when a probe of
    // kTieProbeRows sample rows (batch kernel) finds >= 90 % of them crossing a tie.
    int tieDenseOpt = -1;
    bool tieDense = false;
    bool tieProbed = false;
    DevBuf<uint32_t> d_probeSrc;
    DevBuf<double> d_probeSh;
    DevBuf<double> d_probeSeed;
    int replaySlotsOpt = 0;   // option "replay_slots" (0 = sized from the CUs and free HBM)
    int replayWpc = 20;       // option "replay_wpc": replay wavefronts per CU (LDS and HBM allowing)
    bool rwsInt = false;      // the replay workspace's node block is laid out for u32 keys
    bool replayLandmark = true;  // option "replay_landmark": skip edges into vertices the
                                 // landmark bound proves popped (topo_replay.hip)
    bool replayIntOpt = true;    // option "replay_int_keys": u32 heap keys when replayIntOk
    bool replayIntOk = false;    // every latency an integer and V x max < 2^32 - 1 (upload_replay)
    int sourceOrder = 2;      // option "source_order": batch kernel source grouping (0 = row
                              // order, 1 = by the hub their h0-tree path enters the core, then
                              // pi, 2 = preorder of the h0 shortest-path tree)
    int batchFill = 0;        // option "batch_fill": sources per batch (0 = auto: the fewest per
                              // batch that finish the rows in the same rounds of the slots)
    int batchOrder = 5;       // option "batch_order": 0 grouped order, 1 shuffled, 2 / 3 by mean
                              // pi descending / ascending, 4 by mean h0-tree depth descending,
                              // 5 auto (4 past 3 rounds of the slots, else 2)
    bool targetSkip = true;   // option "target_skip": target bits in the relaxation copy; pairs
                              // into non-target tail vertices that would expand nothing are
                              // dropped (topo_sssp_batch.hip)
    std::vector<uint32_t> adjkTargets;  // the target set whose bits d_adjk carries
    bool leafTargets = true;   // option "leaf_targets": a target with one non-loop edge is resolved
                               // from its uplink (undirected topologies; topo_sssp_batch.hip)
    bool adjkLeaf = false;     // d_adjk's target-derived content is that of the effective target
                               // set: (adjkTargets - peeled) + uplinks, peeled vertices dead
    bool h0Seed = true;        // option "h0_seed": the batch kernel's landmark bound d_j(h0) starts
                               // at the prepared d(s_j, h0) (h0_seed_of) instead of +inf
    std::vector<uint32_t> leafFor;  // the target set d_tleaf / d_tbitsEff / d_dead belong to
    int64_t leafPeeled = 0;         // ... and its peeled targets
    bool adjkFlagged = false;
    bool adjkPlain = false;    // d_adjk / d_kap / d_ksum / d_kap0 are the plain kappa-sorted copy
    bool adjkResorted = false; // ... re-sorted by the target-aware key of adjkTargets
    bool targetResort = true;  // option "target_resort": rows of the relaxation copy re-sorted
                               // by the target-aware key per target set (kappa-prefix cuts stop
                               // before heads that relax nothing reaching a target)
    int targetKappa = 6;      // option "target_kappa": iterations of the target-aware kappa
                              // fixpoint written into the relaxation copy (0: kappa0).  C4 kernel:
                              // 2 iterations 226 ms, 4: 199, 6: 194, 12: 194, 32: 196 (no
                              // fixpoint is reached: cycles without targets rise forever; every
                              // iterate is exact)
    DevBuf<double> d_pot, d_kfA, d_kfB, d_kfPart;
    DevBuf<double> d_kfKap;   // the out-rows' static w - pi(y) of the kappa fixpoint
    const double* kfFinal = nullptr;  // d_kfA or d_kfB: the last iterate [K | Kt] of the target
                                      // preparation d_adjk carries (shdtopo_export_prep)
    bool kfKapReady = false;
    // the target-aware re-sort's scratch (KprimeScratch), kept: the first build's target
    // preparation allocates nothing (the background preparation sizes it)
    DevBuf<float> d_kpKey;
    DevBuf<uint32_t> d_kpIdx;
    DevBuf<uint4> d_kpRec;
    DevBuf<uint8_t> d_kpTmp;
    // the rows longer than kSegBlock (SegBig): their entries' positions and row ordinals, the
    // radix sort's key / value buffers
    DevBuf<uint32_t> d_kpBigPos, d_kpBigRow, d_kpBigVal;
    DevBuf<unsigned long long> d_kpBigKey;
    int64_t kpBig = -1;  // their entries (-1: not listed yet)
    int kpBigBits = 33;
    // the target preparation runs asynchronously (overlapping the host's source order): its
    // iteration count and event time are read after the build's next stream sync
    bool tpPending = false;
    hipEvent_t evp0 = nullptr, evp1 = nullptr;
    // hub rows cut into segments (HubSegs): {row, first entry} and the rows cut in several
    DevBuf<uint2> d_hseg;
    DevBuf<uint4> d_hmulti;
    uint32_t hsegRows = 0, hsegN = 0, hmultiN = 0;
    int slotsUsed = 0;  // workgroups of the last batched launch (<= slots)
    DevBuf<unsigned int> d_kfChanged;
    DevBuf<uint32_t> d_rowmap, d_bsrc;  // batch order: output row and source of each position
    // cache of the last batch order (enqueue_rows): the rows' sources, batch fill and options
    std::vector<uint32_t> ordSrc;
    std::vector<uint32_t> ordBase;  // positions in the grouping order (source_order)
    std::vector<uint32_t> ordPerm;  // ... then batches in batch_order
    bool ordUploaded = false;       // d_rowmap / d_bsrc / d_srcsh hold ordPerm's layout
    const HostPrep* ordHp = nullptr;
    // measured batch layout (option "balance"): per vertex the cost of a
    // source in its batch (wall-clock ticks, EMA over the builds; 0 = none yet), and a batch's
    // fixed cost; the positions' sources and batch starts of the uploaded layout
    int balance = 1;  // 2: costs frozen after the first build (diagnostic)
    int64_t lastBatches = 0;
    std::vector<float> srcCost;
    const HostPrep* costHp = nullptr;
    double costA = 0.0;
    std::vector<uint32_t> layPsrc;
    DevBuf<uint32_t> d_bstart;
    DevBuf<unsigned long long> d_btrace;
    int ordKf = -1, ordSO = -1, ordBO = -1;
    double ordDelta = -1.0;
    double ordPhase = -2.0;
    // option "h0_phase": where the landmark h0 sits in its bucket (the fraction of the bucket
    // below its shifted distance, which is the same for every source).  Unset: h0 closes its
    // bucket with a gap of min(0.01 delta, minLat / 2) to the bucket's end, so no neighbour of h0
    // shares its bucket and the hub core around it is expanded in the next bucket with d(h0)
    // final and the landmark bound tight.  < 0: the round-4 shifts (sh =
    // piMax - pi(s) + 2 delta, h0's phase whatever piMax / delta gives)
    double h0Phase = 0.99;
    bool h0PhaseSet = false;
    bool replayUploaded = false;
    int64_t rnadj = 0;  // entries of the replay CSR
    DevBuf<uint32_t> d_rrow;
    DevBuf<uint4> d_rrec;
    DevBuf<uint32_t> d_rown;
    DevBuf<double2> d_rhop;
    DevBuf<uint32_t> d_tbits;
    // leaf targets (ensure_leaf_targets): the records, the effective target bitmap, the peeled
    // vertices' bitmap, their count
    DevBuf<uint4> d_tleaf;
    DevBuf<uint32_t> d_tbitsEff, d_dead, d_leafCount;
    DevBuf<uint4> d_rvrec, d_rnode;
    DevBuf<uint32_t> d_rpath, d_rrows;
    DevBuf<uint8_t> d_rowflag;
    int rslots = 0;
    int rslotsUse = 0;      // replay wavefronts of the next launch (<= rslots)
    hipEvent_t evr0 = nullptr, evr1 = nullptr;
    bool replayPending = false;

    // route tracing (shdtopo_trace_routes, topo_trace.hip): ids the replay CSR does not carry,
    // uploaded by the first trace -- relabelled -> original vertex, the igraph_get_eid edge of
    // every replay-CSR entry, the lowest-id self loop of every vertex
    int traceChunk = 0;       // option "trace_chunk": sources per replay launch (0 = the slots)
    int traceBatch = 1;       // option "trace_batch": 1 = chains from the batch kernel's pair
                              // records where eligible (prepare_batch_path), 0 = always replay
    bool traceIdsReady = false;
    DevBuf<int32_t> d_tperm, d_reid, d_selfEid;
    ShdTraceStats traceStats{};  // the last trace's own counters
    // link load (shdtopo_link_load, topo_load.hip)
    int loadWalk = 1;            // option "load_walk": 1 = the per-request walk (the default:
                                 // DESIGN.md 3.7), 0 = the leaf-to-root tree accumulation
    ShdLoadStats loadStats{};    // the last call's own counters
    ShdCrossStats crossStats{};  // link crossings (shdtopo_link_crossings, topo_cross.hip)
    ShdTimelineStats timelineStats{};  // link timeline (shdtopo_link_timeline, topo_timeline.hip)
    // link monitors (shdtopo_monitor_*, topo_monitor.hip): {id, monitor}; option
    // "monitor_index_mb" (0 = half of the free device memory at prepare)
    std::vector<std::pair<int, LinkMonitor*>> monitors;
    double monitorIndexMb = 0.0;
    // traffic matrices (shdtopo_matrix_*, topo_matrix.hip): {id, matrix}; option "matrix_mb" (0 =
    // half of the free device memory at a growth; host cells: no cap)
    std::vector<std::pair<int, TrafficMatrix*>> matrices;
    double matrixMb = 0.0;

    // multi-GPU build inside the library (one Shadow process): device d builds
    // rows [d*R, (d+1)*R) with its own stream / workspace (a peer Topology on that device),
    // RCCL all-gathers the rows into every device's table and all-reduces the minimum
    int devicesOpt = 1;        // option "devices"
    int xchgMode = 0;          // option "exchange": 0 auto (RCCL across distinct devices, else
                               // push), 1 RCCL all-gather, 2 push (peer DMA as each shard ends)
    hipStream_t xstream = nullptr;  // exchange stream of a push exchange
    // the getters' row copies (snap_row): a few streams shared by the worker threads, made by
    // dev_init (the background init) so that no query pays a stream creation
    static constexpr int kCopyStreams = 16;
    hipStream_t cstream[kCopyStreams] = {};
    int memShareDiv = 1;       // engines of this build sharing this engine's physical device: its
                               // workspaces take that share of the device's free memory
    bool forceRccl = false;    // option "rccl": the RCCL exchange even with one device (tests)
    std::vector<Topology*> peers;      // devices 1..N-1
    std::vector<ncclComm_t> comms;     // one per device, ncclCommInitAll
    std::vector<int> commDevs;
    int64_t shardRows = 0;

    // host mirror of the table for the per-call getters: an immutable snapshot swapped atomically
    // (getters on worker threads never see a table being rebuilt)
    std::shared_ptr<const HostTable> snap;
    std::atomic<int64_t> rowsToHost{0};      // ShdStats.rows_to_host
    std::atomic<int64_t> rowsToHostNs{0};    // ShdStats.rows_to_host_ms
    double eagerMin = -1.0;

    // attached-set generations: setGen bumps whenever a vertex gains its first or loses its last
    // host (the table's columns change); tableGen = the setGen the device table was built for
    std::atomic<uint64_t> setGen{1};
    std::atomic<uint64_t> tableGen{0};  // written under buildMu, read lock-free by table_current
    std::atomic<uint64_t> tableSerial{0};  // bumps on every device table build / bind
    bool geomInit = false;

    // lazy emulation.  SSSP branch: the reference's cache holds (s, t) iff
    // row s was computed (computeSourcePaths) at a moment t was attached; rows are recomputed on
    // a miss.  Epochs are ipGen values: per vertex the attach intervals [start, end) of "at
    // least one host on it", per source vertex the epochs it was materialised at.
    std::vector<uint32_t> hostsOn;                             // hosts per vertex (ipMu)
    // window adapters registered (shdtopo_window_hold) and the vertices that lost their last
    // host since the last flush: they stay table columns until shdtopo_window_release (ipMu)
    int windows = 0;
    std::vector<int32_t> deferredOff;
    std::unordered_map<int32_t, std::vector<std::pair<uint64_t, uint64_t>>> ivals;  // (ipMu)
    std::atomic<uint64_t> lastNewEpoch{0};                     // latest interval start
    std::unique_ptr<std::atomic<uint64_t>[]> matGen;          // per vertex: latest epoch
    std::unordered_map<int32_t, std::vector<uint64_t>> matEpochs;  // all epochs (lazyMu)
    std::unordered_map<int32_t, double> matMin;  // the row minimum its latest one offered (lazyMu)
    std::mutex lazyMu;
    // per (column pair) bit of the complete branch, for one geometry; superseded arrays stay
    // allocated (getters read the current one without a lock)
    struct PairBits {
        size_t words = 0;
        std::unique_ptr<std::atomic<uint64_t>[]> bits;
    };
    std::atomic<PairBits*> matPair{nullptr};
    std::vector<std::unique_ptr<PairBits>> matPairs;
    std::mutex minMu;
    double lazyMin = 0.0;  // top->minimumPathLatency

    // the reference's shortestPathTotalTime / shortestPathCount (shd-topology.c:46-47,792-793),
    // logged when the topology is freed (:445-446): rows built and the builds' wall time
    double spTotalSec = 0.0;
    uint64_t spCount = 0;

    // stats
    bool rowsPending = false;  // a launch whose stats have not been read back yet
    bool routePending = false;
    ShdStats stats{};
    std::chrono::steady_clock::time_point bstepT;
};

namespace shdtopo {

// Hubs of the tail grouping: the tail is grouped by its highest-ranked neighbour
// among the first kGroupHubs vertices of the degree order (the count the former single-source
// kernel held in LDS, where the grouping was tuned).
constexpr int64_t kGroupHubs = 16565;

// ---- topo_build.cpp: the whole-table build (each holds buildMu) ----
int enqueue_rows(Topology* top, int64_t row0, int64_t row1, double2* out_lr, uint16_t* out_hops,
                 double* out_rowmin, hipStream_t st);
int collect_row_stats(Topology* top);
int build_multi(Topology* top);
int num_devices();
void bstep_mark(Topology* top, int i);
void reset_build_stats(Topology* top);
void plan_long_rows(const uint32_t* rowptr, int64_t V, std::vector<uint32_t>& pos,
                    std::vector<uint32_t>& row, int* end_bit);
int ensure_kprime_scratch(Topology* top, KprimeScratch* out);
// (file-local before the split: hidden, so the library exports what it did)
__attribute__((visibility("hidden"))) bool layout_from_costs(
    const std::vector<double>& c, double a, int kf, int slots, int K, std::vector<uint32_t>& order,
    std::vector<uint32_t>& lstart);
__attribute__((visibility("hidden"))) void release_comms(Topology* top);

// ---- topo_core.cpp: what the table build and the flow analysis call (each holds buildMu) ----
int dev_init(Topology* top);
uint64_t compute_geometry(Topology* top);
int32_t vertex_of_ip(Topology* top, uint32_t ip);
void edge_scan(Topology* top);
Topology* slot_engine(Topology* top, int d);
HubSegs hub_segs(Topology* top);
const uint32_t* adj_out(Topology* top);
void release_workspace(Topology* top);
double h0_phase(Topology* top, double delta);
int upload_csr(Topology* top);
int upload_replay(Topology* top);
int ensure_replay_ws(Topology* top, int nrows);
int upload_target_bits(Topology* top, const std::vector<uint32_t>& tgt, hipStream_t st);
int ensure_workspace(Topology* top, int nsrc);
int hub_rows_ready(Topology* top, uint32_t H, hipStream_t st);
int ensure_leaf_targets(Topology* top, const std::vector<uint32_t>& tgt, const uint32_t* d_tgt,
                        hipStream_t st);
bool leaf_targets_on(const Topology* top);
int batch_k(Topology* top);
int64_t ring_entries(Topology* top, int K);
double default_delta(Topology* top);
SsspLdsPlan batch_lds_plan(Topology* top, int K);
DevCSR dev_csr(Topology* top);
SlotWs slot_ws(Topology* top);
ReplayCSR replay_csr(Topology* top);
ReplayWs replay_ws(Topology* top);
std::vector<double> source_shifts(Topology* top, const uint32_t* s, int64_t n, double delta);
std::vector<double> source_h0_seeds(Topology* top, const uint32_t* s, int64_t n);
// the table of the current attached set: whether it stands, its arrays, and its build
bool table_current(Topology* top);
const double2* tab_lr(const Topology* top);
const uint16_t* tab_hops(const Topology* top);
int ensure_table(Topology* top);
// ... and what a derived topology is made with (shdtopo_derive_without, topo_whatif.cpp): the
// graph checks of a new topology (nullptr: it was freed), its background device init and graph
// preparation, one host onto vertex v
Topology* finish_new(Topology* top);
void start_device_init(Topology* top);
void start_graph_prep(Topology* top, bool onLoad);
void do_attach(Topology* top, uint32_t ip, int32_t v, uint64_t* bwDownOut, uint64_t* bwUpOut);

// the *_stats getters: the last call's counters, under the build lock
template <class S>
int copy_stats(Topology* top, S _Topology::*field, S* out) {
    if (!top || !out) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    *out = top->*field;
    return 0;
}

// ---- topo_monitor_host.cpp ----
void monitors_release(Topology* top);

// ---- topo_matrix_host.cpp ----
void matrices_release(Topology* top);

// ---- topo_flows.cpp: the parts of the flow analysis the link monitor shares ----

// the packet kernel's conversion (topo_kernels.hip): milliseconds -> nanoseconds, rounded up
inline uint64_t lat_ns(double ms) { return (uint64_t)std::ceil(ms * 1000000.0); }

// The binning rule of the timeline and the monitors: weight w of a hit at t on row goes to its bin
// of bins (rows x nbins) or to the row's outside pair.  0: before t0, 1: in range, 2: after.
inline int bin_add(uint64_t t0, uint64_t binNs, int64_t nbins, uint64_t* bins, uint64_t* outside,
                   int64_t row, uint64_t t, uint64_t w) {
    if (t < t0) {
        if (outside) outside[2 * row] += w;
        return 0;
    }
    if (nbins > 0 && (t - t0) / binNs < (uint64_t)nbins) {
        bins[row * nbins + (int64_t)((t - t0) / binNs)] += w;
        return 1;
    }
    if (outside) outside[2 * row + 1] += w;
    return 2;
}

// The requests' vertices: both ends on a vertex of the current attached set, else -1; returns the
// requests with both.
int64_t resolve_requests(Topology* top, const uint32_t* srcIP, const uint32_t* dstIP, int64_t n,
                         std::vector<int32_t>& sv, std::vector<int32_t>& dv);

// the watch lists and the bin geometry of a timeline call or a monitor; *rows = 2 ne + nv
bool watch_bins_ok(Topology* top, const int32_t* watchEdge, int64_t ne, const int32_t* watchVertex,
                   int64_t nv, uint64_t binNs, int64_t nbins, int64_t* rows);

// the igraph_get_eid edge (lowest id; -1 = none) of every (sv[i], dv[i]) with both ends attached
std::vector<int32_t> complete_pair_eids(Topology* top, const std::vector<int32_t>& sv,
                                        const std::vector<int32_t>& dv, int64_t n);

// a trace leaves the last build's statistics and the replay's launch width as they were
struct TraceKeep {
    Topology* top;
    ShdStats stats;
    int rslotsUse;
    explicit TraceKeep(Topology* t) : top(t), stats(t->stats), rslotsUse(t->rslotsUse) {}
    ~TraceKeep() {
        top->stats = stats;
        top->rslotsUse = rslotsUse;
    }
};
// 0 / 1 bracket a chunk's replay launch, 2 closes the chunk; 3 / 4 bracket its keep launch, 5 / 6
// the pair walks' first pass
using TraceEvents = DevEvents<7>;

// The requests of a trace or a link load grouped for the replay: those with both ends attached,
// sorted by source (stable: request order within a source), a CSR over the distinct sources and
// each source's slot within its chunk, uploaded; the replay's CSR and workspace for the table
// build's target set; the events that time a chunk.
struct ReplayReqs {
    std::unique_ptr<TraceKeep> keep;  // declared first: ShdStats and the launch width go back last
    std::vector<uint32_t> order, srcs, srcStart;
    size_t nv = 0, mmax = 0;  // grouped requests; the most of one chunk
    int nsrc = 0, chunk = 0;
    ReplayCSR csr;
    ReplayWs ws;
    TraceIds ids;
    DevBuf<uint32_t> d_srcs, d_rslot, d_rsrc, d_rdst, d_ridx;
    DevBuf<unsigned long long> d_st;  // its own counters: the last build's stay intact
    TraceEvents ev;
    // The batch path (option "trace_batch", prepare_batch_path): a chunk's sources first run the
    // batch kernel's keep launch, kf per batch and slot; the sources whose row it leaves
    // unflagged are walked from the slots' pair records, the others replayed.  Everything the
    // launch writes besides the batch workspace is the call's: targets, shifts, row flags, stats.
    bool batchOk = false;
    int K = 0, kf = 0;
    double delta = 0.0;
    SsspLdsPlan plan;
    DevCSR bcsr;
    SlotWs bws;
    PairChains pc;
    DevBuf<uint32_t> d_tgt, d_rmap, d_fsrcs;
    DevBuf<double> d_srcsh, d_h0seed;
    DevBuf<uint8_t> d_rowflag, d_broken;
    DevBuf<unsigned long long> d_bst;
    // one chunk's chains (chunk_chains): rmap[i] of chunk source i, the sources replayed
    std::vector<uint32_t> rmap;
    bool mixed = false;  // the chunk ran a keep launch: its requests carry rmap
    int nfall = 0;       // sources of the chunk that were replayed
    TraceReqs reqs(int s0, int s1) const {
        const size_t q0 = srcStart[(size_t)s0];
        return TraceReqs{(int64_t)(srcStart[(size_t)s1] - q0), d_rslot.p + q0, d_rsrc.p + q0,
                         d_rdst.p + q0, d_ridx.p + q0};
    }
};

// The watch set of one call: the ids of each list ascending with their watch index (edges k,
// vertices ne + k; original vertex ids).  false: an id out of range or twice in its list.
struct WatchSet {
    std::vector<int32_t> eids, eidx, vids, vidx;
    static bool sorted_ids(const int32_t* id, int64_t n, int64_t limit, int32_t idx0,
                           std::vector<int32_t>& ids, std::vector<int32_t>& idx) {
        std::vector<std::pair<int32_t, int32_t>> s((size_t)n);
        for (int64_t k = 0; k < n; k++) {
            if (id[k] < 0 || (int64_t)id[k] >= limit) return false;
            s[(size_t)k] = {id[k], (int32_t)(idx0 + k)};
        }
        std::sort(s.begin(), s.end());
        ids.resize((size_t)n);
        idx.resize((size_t)n);
        for (size_t k = 0; k < (size_t)n; k++) {
            if (k > 0 && s[k].first == s[k - 1].first) return false;
            ids[k] = s[k].first;
            idx[k] = s[k].second;
        }
        return true;
    }
    bool init(const HostGraph& g, const int32_t* we, int64_t ne, const int32_t* wv, int64_t nv) {
        return sorted_ids(we, ne, g.E, 0, eids, eidx) &&
               sorted_ids(wv, nv, g.V, (int32_t)ne, vids, vidx);
    }
    static int32_t find(const std::vector<int32_t>& ids, const std::vector<int32_t>& idx,
                        int32_t x) {
        const auto it = std::lower_bound(ids.begin(), ids.end(), x);
        return it != ids.end() && *it == x ? idx[(size_t)(it - ids.begin())] : -1;
    }
    int32_t edge(int32_t e) const { return find(eids, eidx, e); }
    int32_t vertex(int32_t v) const { return find(vids, vidx, v); }
};

// The device image of a watch set (CrossWatch, its totals aside): bits by edge id and by
// relabelled vertex, the sorted ids for the hits.
struct DevWatch {
    DevBuf<uint32_t> d_ebits, d_vbits;
    DevBuf<int32_t> d_eids, d_eidx, d_vids, d_vidx;
    CrossWatch cw;
    int upload(Topology* top, const WatchSet& wset);
};

// sv / dv: the requests' vertices (-1 = not attached).  Prepares the device, the replay and the
// edge ids (*ids_ms), and fills R.  forLoadTree: a link load with the tree accumulation.
int group_replay_requests(Topology* top, const std::vector<int32_t>& sv,
                          const std::vector<int32_t>& dv, int64_t n, double* ids_ms,
                          bool forLoadTree, ReplayReqs& R);

// what a chunked call reports, and its copy into an ABI struct (kernel: the struct's name for
// kernel_ms; ids_ms is the caller's: a monitor has none)
struct ChainStats {
    double replay_ms = 0, kernel_ms = 0, batch_ms = 0, ids_ms = 0;
    int64_t batch_sources = 0, batch_fallback = 0, chunks = 0, sources = 0;
    template <class S>
    void out(S* s, double S::*kernel) const {
        s->replay_ms = replay_ms;
        s->*kernel = kernel_ms;
        s->batch_ms = batch_ms;
        s->batch_sources = batch_sources;
        s->batch_fallback = batch_fallback;
        s->chunks = chunks;
        s->sources = sources;
    }
};

// One chunk of R's sources: [s0, s1), its m requests from q0 of the grouped order (rq; after the
// chains are there it carries rmap), and whether some of them walk the batch kernel's pair records.
struct Chunk {
    int s0 = 0, s1 = 0;
    size_t q0 = 0, m = 0;
    TraceReqs rq;
    bool pairs = false;
};
using ChunkFn = std::function<int(Chunk&)>;

// The chunk driver.  run_chunk: the chunk's m + 1 entries of d_zero zeroed (if given: the caller's
// per-request counts), the chains (chunk_chains; first: the caller's first pass over the pair
// records), body (the caller's walks), the closing event R.ev.e[2], the stream sync, the chunk's
// event times into cs and its count.  for_chunks: every chunk of R in order.
int run_chunk(Topology* top, ReplayReqs& R, int s0, int s1, ChainStats& cs, int64_t* d_zero,
              const ChunkFn& first, const ChunkFn& body);
int for_chunks(Topology* top, ReplayReqs& R, ChainStats& cs, int64_t* d_zero, const ChunkFn& first,
               const ChunkFn& body);

// The validated walk of link load, crossings, timeline and the monitor index: the requests'
// weights (and emission times) in grouped order, the hops the validation leaves for the walks,
// its counters -- d_cnt for the replayed sources over the whole call, d_pcnt for a chunk's pair
// records (a validation that finds a broken chain is run again without that source), read back
// per chunk and summed on the host.
struct Walk {
    DevBuf<unsigned long long> d_w, d_now, d_cnt, d_pcnt;
    DevBuf<int32_t> d_hops;
    size_t ones = 0;  // leading entries of d_w known to be 1 (calls without weights)
    std::deque<std::array<unsigned long long, LD_COUNT>> pcnt;  // per chunk with pair walks
    unsigned long long cnt[LD_COUNT] = {};
    // the uploads (blocking); now only with times
    int upload(const ReplayReqs& R, const uint64_t* weight, const uint64_t* now, bool times);
    int zero(hipStream_t st);  // d_cnt
    ChunkFn first(ReplayReqs& R, hipStream_t st);
    // in a chunk's body: the pair validation's counters start home before the pair walks; the
    // replayed sources' validation before theirs
    int pairs_counted(const Chunk& ck, hipStream_t st);
    int validate(ReplayReqs& R, const Chunk& ck, hipStream_t st);
    unsigned long long total(int i) const {
        unsigned long long t = cnt[i];
        for (const auto& c : pcnt) t += c[(size_t)i];
        return t;
    }
    int64_t routed() const { return (int64_t)total(LD_ROUTED); }
    int64_t broken() const { return (int64_t)total(LD_BROKEN); }
};

// A link load's sums on the device, caller-owned: d_eload u64 [2 E] by document edge id (the
// forward halves, then the reverse halves), d_vout u64 [V] by original vertex id.
struct LoadSums {
    DevBuf<unsigned long long> d_eload, d_vout;
};
// The link load of an SSSP topology in two steps (shdtopo_link_load runs both; the load shift of
// topo_whatif.cpp runs the first on each side and compares on the device).  load_accumulate: the
// sums of the requests (sv / dv: their vertices, -1 = not attached) into `sums`, complete when it
// returns (the stream is synchronised), and routed / broken / hop_weight / tree_vertices into ls.
// load_copy_out: the sums to the host arrays (either may be NULL).  Each holds buildMu.
int load_accumulate(Topology* top, const std::vector<int32_t>& sv, const std::vector<int32_t>& dv,
                    const uint64_t* weight, int64_t n, LoadSums& sums, ShdLoadStats* ls,
                    ChainStats& cs);
int load_copy_out(Topology* top, const LoadSums& sums, uint64_t* edgeLoad, uint64_t* vertexLoad);
// a complete topology's link load, on the host from the parsed graph (adds into edgeLoad u64
// [2 E] / vertexLoad u64 [V], either may be NULL; routed / broken / hop_weight into ls)
int64_t load_complete(Topology* top, const std::vector<int32_t>& sv, const std::vector<int32_t>& dv,
                      const uint64_t* weight, int64_t n, uint64_t* edgeLoad, uint64_t* vertexLoad,
                      ShdLoadStats* ls);

}  // namespace shdtopo
