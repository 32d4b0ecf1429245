// topo_device.h -- device data layout and kernel launchers (implemented in topo_kernels.hip).
//
// HBM layout (all arrays in the degree-relabelled vertex order, see DESIGN.md "Data layout"):
//   CSR of the undirected topology without self loops:
//     rowptr u32[V+1], adj {u32 col, u32 pi / kappa0 field, f64 latency}[2E'] (16-B AoS), its
//     kappa-sorted copy adjk, aloss f64[2E'] (edge loss)
//   per vertex: vloss f64[V], selfLat f64[V] (NaN = no self loop), selfLoss f64[V], pi f64[V]
//   per SSSP slot (one workgroup = K sources at a time): DESIGN.md 3.2
//   routing table: {f64 lat, f64 rel}[A][A] (16-B records, one gather per packet) + u16 hops
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace shdtopo {

#ifndef SHD_SSSP_BLOCK
#define SHD_SSSP_BLOCK 1024
#endif
constexpr int kSsspBlock = SHD_SSSP_BLOCK;  // threads per SSSP workgroup
#ifndef SHD_BATCH_WGPCU
#define SHD_BATCH_WGPCU 1
#endif
constexpr int kBatchWgPerCu = SHD_BATCH_WGPCU;  // batch-kernel workgroups per CU (share its LDS)
constexpr int kMaxHops = 48;      // per-thread path buffer depth (longer paths: O(h^2) walk)
// doubles of the batch kernel's path buffer per slot: the chain losses [kMaxHops][kSsspBlock]
constexpr size_t kPathBufPerSlot = (size_t)kMaxHops * kSsspBlock;
// parent pass: pairs of one row-scan chunk by default (records per slot: chunk x K, one per
// merged vertex and source; C4 sends ~2.6 k pairs per level of a batch to row scans)
constexpr uint32_t kRowScanCap = 16384;
// the candidate count of a row-scan record no pair asked for
constexpr uint32_t kRsUnreq = 0xFFFFFFFEu;
#ifndef SHD_KAP_IN_REC
#define SHD_KAP_IN_REC 1
#endif
// 1: the adjacency record's 32-bit field holds {f16 pi(col) rounded up, f16 kappa0(col) rounded
// down} (high, low half), so the batch relaxation gets the target's kappa0 with the record
// instead of a random 4-B load per surviving edge; 0: f32 pi(col) rounded up, kappa0 from g.kap0
constexpr bool kKapInRec = SHD_KAP_IN_REC != 0;
#ifndef SHD_KPROBES
#define SHD_KPROBES 8
#endif
// kappa probes per vertex (4 or 8): the batch kernel's cut of a kappa-sorted row needs a
// binary search (dependent loads) only past the last probe
constexpr int kKProbes = SHD_KPROBES;
static_assert(kKProbes == 4 || kKProbes == 8, "kappa probes");

// indices into the device stats block (unsigned long long[16])
enum StatIdx {
    ST_GLOBAL_MIN = 0,  // f64 bits of the min latency over every computed pair
    ST_AMBIGUOUS = 1,   // pairs whose parent chain crosses a d-tied parent
    ST_RELAX = 2,       // edge relaxations attempted
    ST_LONGPATH = 3,    // pairs longer than kMaxHops
    ST_ERRORS = 4,      // pairs with a missing edge / unreachable target
    ST_DEQUEUE = 5,     // next source to take (persistent workgroups)
    ST_OVERFLOW = 6,    // queue overflow / iteration guard tripped
    ST_T_INIT = 7,      // wall-clock ticks summed over workgroups: distance init
    ST_T_SSSP = 8,      //   near-far SSSP
    ST_T_PARENT = 9,    //   parent derivation for the target chains
    ST_T_TARGET = 10,   //   per-target latency / reliability / hops
    ST_NEAR_IT = 11,    // near-phase iterations
    ST_SPLITS = 12,     // buckets taken from the bucket window
    ST_EV0 = 13,        // event counters (ShdStats.events): queue entries expanded, tail
                        // relaxations, tail improvements, window entries taken, overflow entries
                        // refilled, parent-pass vertices, relaxations onto settled tail vertices,
                        // stale entries skipped
    ST_FARSCAN = 21,    // sources that overflowed a queue (finished with scanning buckets)
    ST_T_SPLIT = 22,    // wall-clock ticks summed over workgroups: bucket changes + refills
    ST_OVERSITE = 23,   // OR of the push sites that overflowed (diagnostic)
    ST_RP_DEQUEUE = 24, // heap replay: next row to take (persistent wavefronts)
    ST_RP_POPS = 25,    //   heap pops (delete_max) summed over replayed rows
    ST_RP_PUSH = 26,    //   pushes (first reach)
    ST_RP_MOD = 27,     //   modifies (strict improvement of a queued vertex)
    ST_RP_ROWS = 28,    //   rows replayed
    ST_ROUTE_BAD = 29,  // packets with a column outside [0, A) (not routed) since the last build
    ST_PT0 = 30,        // batch kernel parent pass, wall ticks summed over workgroups: walks,
                        //   merged row scans, recount + finalize, next level (4 slots)
    ST_RP_L0 = 34,      // replay 64-B lines (SHD_RP_LINES builds): sink ld/st, shift-up ld/st,
                        // relaxation ld/st
    ST_RP_T0 = 40,      // replay wall ticks (SHD_RP_TIME builds): sink, loads, heap ops, rest
                        // + sink rounds, heap size summed over pops, sink sub-phases
                        // (LDS walk, HBM rounds, moves), root-prefetch hits
    ST_RP_SKIP = 50,    // replay relaxations whose vertex record the landmark skip did not read
    ST_BT0 = 51,        // batch kernel (SHD_BATCH_TIME builds): wave ticks of tail iterations in
                        // chunk loads / phase A / phase B, the same for hub iterations, phase-B
                        // rounds, surviving edges (8 slots)
    ST_TOUCHED = 59,    // tail distance lines reset at batch starts (lines the batches touched)
    ST_WALK = 60,       // batch kernel parent pass: walk steps (pairs claimed and resolved)
    ST_WK0 = 61,        //   of which resolved by the h0-tree guess, by a tail's improver, by a
                        //   hub's improver, and pairs sent to row scans (4 slots)
    ST_SW0 = 65,        // batch kernel sweeps (SHD_BATCH_TIME builds): pending tail vertices
                        //   visited, of which queued (a pair in the opened bucket), holding a
                        //   pair in that bucket that the kappa test kept out, kept pending
    ST_WL0 = 69,        // batch kernel (SHD_BATCH_WRCOUNT builds): 64-B lines written per
                        //   category (16 slots, topo_sssp_batch.hip WL_*)
    ST_RL0 = 85,        //   then 64-B lines read per category (8 slots, RL_*)
    ST_COUNT = 93
};

// A directed topology (igraph mode OUT, shd-topology.c:762-763) relaxes out-edges but finds a
// vertex's parent among its in-edges: rowptr / adjk / kap / ksum / kap0 are the OUT rows,
// rowptr_in / adj / aloss the IN rows (the parent pass).  Undirected: rowptr_in == rowptr.
struct DevCSR {
    int32_t V = 0;
    int64_t nadj = 0;
    const uint32_t* rowptr = nullptr;     // rows of adjk (relaxation)
    // 16-B AdjRec {u32 col, {f16 pi(col) rounded up, f16 kappa0(col) rounded down} (high, low
    // half; kKapInRec = 0: f32 pi(col) rounded up), f64 w}, rows ascending by (neighbour, edge
    // id).  Directed: the in-rows, whose field is not written (0); the out-rows' records with
    // the field exist only as adjk's source
    const uint32_t* adj = nullptr;
    // the relaxation records: the out-rows' AdjRec, each row stably sorted by f32 kappa = w -
    // pi(col) rounded down (from neighbour order), or for a target set by the target-aware key
    // (from that order; the low half of the field is then f16 K(col) rounded down, +inf kept).
    // Column word: bit 31 = the row is the column's h0-tree parent, bit 30 = target mark (tflags)
    const uint32_t* adjk = nullptr;
    const float* kap = nullptr;     // adjk's sort key (f32 rounded down; -inf: pi unknown)
    const float4* ksum = nullptr;   // per vertex: kappa at row positions 0, 1, 3, 7[, 15, 31, 63,
                                    // 127] (kKProbes floats, +inf past the row)
    const float* kap0 = nullptr;    // per vertex: smallest kappa of its row (+inf: empty row)
    // per vertex, 32 B: {h0-tree parent, the adjacency position (into adj / aloss) of the
    // parent's first entry in v's row (in-row when directed), f64 w, f64 packet loss of that
    // edge, pad} (one line per walk hop); h0: {~0, ~0, ~0, ~0, 0...}
    const uint32_t* spt = nullptr;
    double piMax = 0.0;             // largest finite pi
    const double* aloss = nullptr;
    const double* vloss = nullptr;
    const double* selfLat = nullptr;
    const double* selfLoss = nullptr;
    int rows_sorted = 0;  // adjacency rows ascending by neighbour (enables binary row search)
    // bit 30 of adjk's column word marks an attached vertex (a table target); the batch
    // relaxation then skips pairs into non-target tail vertices that would expand nothing.
    // 2: the marks are the effective target set's (leaf targets peeled, SlotWs::tleaf) and a
    // record whose kappa field is +inf leads to a dead vertex: its pairs are dropped outright
    int tflags = 0;
    // (last: the undirected kernel's argument layout stays that of the fields above)
    int directed = 0;
    const uint32_t* rowptr_in = nullptr;  // rows of adj / aloss (parent pass)
};

// per-slot workspace of the batched SSSP (sssp_batch_kernel, K sources per slot), slot-major:
// array + slot * V [* K]
struct SlotWs {
    int slots = 0;
    int64_t V = 0;
    unsigned long long* dist = nullptr;  // [V][K] f64 bits, +inf = unreached (rows < H unused)
    uint4* prec = nullptr;               // [V][K] pair records {parent | amb << 31 | bad << 30,
                                         // batch tag, f64 loss of the parent edge}
    unsigned long long* qa = nullptr;    // near queues / parent pair lists (q_stride u64 per slot)
    unsigned long long* qb = nullptr;
    uint32_t* ring = nullptr;            // ring_entries u32 per slot: parent pair list, vertex
                                         // list, pending bitmap, tie bitmap
    uint4* rscan = nullptr;              // parent pass, rs_chunk x K per slot: per (merged vertex,
                                         // source) of a row-scan chunk {min d[u] over the candidates
                                         // (u64), candidates at the min, lowest adjacency slot}
    uint32_t rs_chunk = kRowScanCap;     // pairs per row-scan chunk (option "row_scan_chunk")
    double* pathbuf = nullptr;           // [slot][kPathBufPerSlot]: edge losses of a path
    uint32_t* counters = nullptr;        // [slot][4]: batch tag, (unused)
    int K = 8;
    int64_t q_stride = 0;
    int64_t ring_entries = 0;
    uint8_t* mask = nullptr;             // 2 parities of a K-bit source mask per vertex
    uint32_t* hpar = nullptr;            // [P][K] parent hints of the LDS hubs
    // per row of the launch: set to 1 when a pair of the row crosses a d-tied parent (its parent
    // chain needs igraph's heap pop order: the row is recomputed by heap_replay_kernel)
    uint8_t* rowflag = nullptr;
    // output row of batch position p (sources are taken in a locality order, the table keeps
    // row order); nullptr = identity
    const uint32_t* rowmap = nullptr;
    // diagnostic (SHD_BATCH_TRACE): per batch kBTraceWords u64 {wall_clock64 at dequeue, at its
    // end, slot, near iterations, sweeps, expansions, relaxations, sources, ticks at the SSSP's,
    // the parent pass' and the epilogue's end, 0}
    unsigned long long* btrace = nullptr;
    // batch layout (option balance, topo_core.cpp): batch b takes positions [bstart[b],
    // bstart[b + 1]) (at most K), nbat batches; nullptr = batch b takes [b kf, b kf + kf)
    const uint32_t* bstart = nullptr;
    int nbat = 0;
    // leaf-target records (option "leaf_targets", launch_leaf_targets), 32 B per target k:
    // {targets[k], uplink u (kNoLeaf: not peeled), f64 w} {f64 loss of the edge (u, t), 0, 0}.  A
    // peeled target is resolved from its uplink: d(t) = fl(d(u) + w), parent(t) = u.  nullptr: no
    // target is peeled (the kernel reads targets[k] alone)
    const uint4* tleaf = nullptr;
};
constexpr uint32_t kNoLeaf = 0xFFFFFFFFu;
constexpr int kBTraceWords = 12;  // u64 words per batch of SlotWs::btrace (per-batch trace / costs)

// Incidence-order CSR of the heap replay (topo_replay.hip), relabelled vertex ids: row x holds
// x's neighbours in igraph_incident order (ascending ORIGINAL neighbour id; directed graphs:
// out-neighbours), self loops dropped, parallel edges merged.
//   rec  {u32 col, u32 row vertex x, f64 latency (min over a parallel group)}   16 B
//   hop  {f64 latency, f64 packet loss} of the igraph_get_eid edge (lowest edge id)  16 B
struct ReplayCSR {
    int32_t V = 0;
    int64_t nadj = 0;
    const uint32_t* rowptr = nullptr;
    // {u32 neighbour, f32 pi(neighbour) rounded up (+inf: no landmark), f64 w} per entry
    const uint4* rec = nullptr;
    const uint32_t* own = nullptr;  // row (vertex) of each entry: the epilogue's parent walk
    const double2* hop = nullptr;
    const double* vloss = nullptr;
    const double* selfLat = nullptr;
    const double* selfLoss = nullptr;
    const uint32_t* tbits = nullptr;  // target (attached vertex) bitmap over V
    int64_t ntargets = 0;             // distinct targets (igraph's to_reach)
    int32_t landmark = -1;            // vertex the rec pi values are measured from (-1: none)
    // 1: u32 heap keys (every latency an integer, V x max latency < 2^32 - 1: exact, see
    // topo_replay.hip RpKey); 0: f64 keys
    int32_t intKeys = 0;
};

// per-slot workspace of the heap replay (one wavefront = one slot), slot-major [slot][V]:
// vertex records {f64 dist (-1 = unreached), u32 parent (replay-CSR slot of the parent edge),
// u32 heap position} and heap nodes {f64 key, u32 vertex, pad} (positions >= the LDS part),
// 16 B each (one line per access; u32 keys: {u32 dist, pad, ...} and 8-B nodes {u32 key, u32
// vertex}, the node block then V x 8 B per slot), and a path buffer [kMaxHops][64] per slot.
// 32 B (u32 keys: 24 B) x V + 12 KiB per slot.
struct ReplayWs {
    int slots = 0;
    uint4* vrec = nullptr;
    uint4* node = nullptr;     // nodeCap heap nodes per slot (node size: 8 B u32 keys, 16 B f64)
    uint32_t* pathbuf = nullptr;
    uint32_t nodeCap = 0;      // physical heap nodes per slot (replay_layout)
    uint32_t stdPos = 0;       // first heap position stored position-major (past the blocked bands)
    uint32_t stdBase = 0;      // its physical node index
};
// Physical layout of a replay heap's HBM levels (topo_replay.hip, RpHeap::phys): the levels below the
// LDS ones in bands of one sink round's height, each band root's subtree contiguous; the levels
// past the last band the heap can fill, position-major.
struct ReplayLayout {
    uint32_t stdPos, stdBase, nodeCap;
};
ReplayLayout replay_layout(int int_keys, uint32_t V);

// Hub rows (ids < rows: the long rows of the degree order) cut into segments of at most kHubSeg
// entries, one wavefront each in the row-parallel steps (graph preparation, the target-aware
// kappa fixpoint): the longest rows (250 k entries on C4) no longer serialise on one wavefront.
// A row cut into several segments leaves one partial result per segment, combined by a
// finalize pass over `multi`.
constexpr uint32_t kHubSeg = 4096;
struct HubSegs {
    uint32_t rows = 0;             // hub rows [0, rows); the rest take a thread each
    const uint2* seg = nullptr;    // {row, first entry} per segment, rows ascending
    uint32_t nseg = 0;
    const uint4* multi = nullptr;  // {row, first segment, segments, 0} of the rows cut in several
    uint32_t nmulti = 0;
};
// the segment tables of rows [0, rows) from the first rows + 1 entries of rowptr (host)
void hub_segments(const uint32_t* rowptr_head, uint32_t rows, std::vector<uint2>& seg,
                  std::vector<uint4>& multi);

// LDS plan of one batched SSSP workgroup: H hub distance rows (+ their queue masks) and P
// parent hints, sized to the CU's 160 KiB.
struct SsspLdsPlan {
    uint32_t H = 0;     // LDS-resident hub distances (vertex ids 0..H-1 after the relabel)
    uint32_t P = 0;     // hubs with parent hints (P <= H)
    size_t bytes = 0;   // dynamic LDS per workgroup
};

// Batched multi-source SSSP (topo_sssp_batch.hip): K in {2, 4, 8, 16} sources per workgroup in
// lock-step over buckets of d + srcsh[row] (srcsh >= 2 delta).  plan from sssp_batch_lds_plan.
// kf (1..K): sources per batch (batch b = positions [b kf, b kf + kf)).
SsspLdsPlan sssp_batch_lds_plan(int K, int64_t hub_limit, uint32_t par_hubs, int64_t V);
// bit 30 of every adjk column word := the column is set in tbits (the attached vertices)
hipError_t launch_mark_targets(uint32_t* adjk, int64_t nadj, const uint32_t* tbits,
                               hipStream_t stream);
// target-aware kappa fixpoint (topo_sssp_batch.hip): kap_e = every out-row entry's w - pi(y)
// (static: once per graph); one step K_out = F(K_in) (K_in nullptr: kappa0), K buffers of 2 V
// doubles [K | Kt = target ? -inf : K]; then the f16 kappa field of the relaxation copy's records
// := K(column).  part: scratch of hs.nseg doubles (the per-segment minima of cut rows)
hipError_t launch_kfix_kap(const uint32_t* adj, const double* pot, int64_t nadj, double* kap,
                           hipStream_t stream);
// dead (nullable): bitmap of the peeled leaf targets, whose K and Kt are forced to +inf (the edge
// into one sorts past every kappa cut and the pair skip drops it)
hipError_t launch_kfix_step(const uint32_t* rowptr, const uint32_t* adj, const double* kap_e,
                            const uint32_t* tbits, const double* Kin, double* Kout, int64_t V,
                            const HubSegs& hs, double* part, unsigned int* changed,
                            hipStream_t stream, const uint32_t* dead = nullptr);
// Leaf targets of an undirected simple topology (rows without self loops): target k is peeled
// when its row has exactly one entry (u, w) and u's row has more than one (of two mutually
// pendant vertices neither is peeled).  Writes the SlotWs::tleaf record of every target, turns
// tbits (in: the targets' bitmap) into the effective target set (targets - peeled) + {uplinks of
// peeled}, sets the peeled vertices in dead (in: zero) and adds their number to *count.
hipError_t launch_leaf_targets(const uint32_t* rowptr, const uint32_t* adj, const double* aloss,
                               const uint32_t* targets, int A, uint4* tleaf, uint32_t* tbits,
                               uint32_t* dead, uint32_t* count, hipStream_t stream);
hipError_t launch_kfix_store(uint32_t* adjk, int64_t nadj, const double* K, hipStream_t stream);
// re-sort every row of the relaxation copy (records, kappa array, probes, kappa0) by the
// target-aware key kap' of the current target set (tbits) and K.  Scratch (KprimeScratch, sized
// by kprime_scratch_bytes) is the caller's, so the resort allocates nothing and never syncs.
// rows of at most kSegBlock entries are sorted in LDS; the longer ones' entries, listed once per
// graph row by row (pos: adjacency position, row: the row's ordinal among the long rows), go
// through a device-wide radix sort of (ordinal << 32 | key) -- end_bit = 32 + bits of the ordinal
constexpr uint32_t kSegBlock = 4096;
struct SegBig {
    const uint32_t* pos = nullptr;
    const uint32_t* row = nullptr;
    int64_t nitems = 0;
    int end_bit = 33;
    unsigned long long* keys = nullptr;  // 2 x nitems
    uint32_t* vals = nullptr;            // 2 x nitems
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
};
struct KprimeScratch {
    float* key = nullptr;       // nadj
    uint32_t* idx = nullptr;    // nadj: each sorted entry's source position
    uint4* rec = nullptr;       // nadj
    SegBig big;                 // the rows longer than kSegBlock (listed once per graph)
};
// segmented sort (ascending f32 keys, stable, hipcub's order): rows <= 64 by waves, <= kSegBlock
// by workgroups in LDS, the longer rows' entries by one device-wide radix sort
hipError_t segsort_big_tmp_bytes(int64_t nitems, int end_bit, size_t* bytes);
hipError_t launch_segsort(const uint32_t* rowptr, int64_t V, int64_t nadj, const float* key,
                          float* key_out, uint32_t* idx_out, const SegBig& big, hipStream_t stream);
hipError_t segsort_reference(const uint32_t* rowptr, int64_t V, int64_t nadj, const float* key,
                             const uint32_t* idx_in, float* key_out, uint32_t* idx_out, void* tmp,
                             size_t* tmp_bytes, hipStream_t stream);
hipError_t preload_kprime_sort(hipStream_t stream);
hipError_t launch_kprime_resort(uint32_t* adjk, float* kap, float* ksum, float* kap0,
                                const uint32_t* rowptr, int64_t V, int64_t nadj, const double* pot,
                                const uint32_t* tbits, const double* K, const KprimeScratch& sc,
                                hipStream_t stream);
hipError_t launch_sssp_batch(int K, const DevCSR& g, const SlotWs& ws, const uint32_t* d_sources,
                             const double* d_srcsh, const double* d_h0seed, int nsrc, int kf,
                             const uint32_t* d_targets, int A,
                             double delta, const SsspLdsPlan& plan, uint32_t iter_guard,
                             double2* out_lr, uint16_t* out_hops, double* out_rowmin,
                             unsigned long long* d_stats, hipStream_t stream);
// The keep launch (sssp_batch_kernel<K, DIR, true>): block b runs batch b = positions [b kf,
// b kf + kf) once in slot b, so (nsrc + kf - 1) / kf <= ws.slots; a bstart layout and btrace are
// rejected.  SSSP, parent pass and epilogue are the build's (ws.rowflag[position], ST_ERRORS and
// ST_LONGPATH in d_stats -- the caller's own block, zeroed by it), but no table is written.
// Afterwards slot b's pair records tagged ep | kPairTagClaim, ep = (counters[4 b] - 1) %
// kPairTagMask + 1, are the parent chains of batch b: lane j of vertex v at prec[slot][v K + j].
hipError_t launch_sssp_batch_keep(int K, const DevCSR& g, const SlotWs& ws,
                                  const uint32_t* d_sources, const double* d_srcsh,
                                  const double* d_h0seed, int nsrc, int kf,
                                  const uint32_t* d_targets, int A, double delta,
                                  const SsspLdsPlan& plan, uint32_t iter_guard,
                                  unsigned long long* d_stats, hipStream_t stream);
// tag word of a pair record (topo_sssp_batch.hip): the batch tag | claim bit of a resolved pair
constexpr uint32_t kPairTagMask = 0x3FFFFFFFu;
constexpr uint32_t kPairTagClaim = 0x40000000u;

// Exact igraph-0.7 Dijkstra replay, one wavefront per row (topo_replay.hip): rows[0..nrows) index
// d_sources / the output rows.  full = 1 ignores the early exit (test hook); dbg_dist / dbg_par
// (V entries, nrows == 1) receive the replay's distances and parent vertices (relabelled ids).
hipError_t launch_heap_replay(const ReplayCSR& g, const ReplayWs& ws, const uint32_t* d_sources,
                              const uint32_t* d_rows, int nrows, const uint32_t* d_targets, int A,
                              int full, double2* out_lr, uint16_t* out_hops, double* out_rowmin,
                              unsigned long long* d_stats, double* dbg_dist, int32_t* dbg_par,
                              hipStream_t stream);
int replay_lds_levels(int int_keys);
int replay_lds_bytes(int int_keys);  // LDS of one replay wavefront (its heap's top levels)

// ---- route tracing (topo_trace.hip): the vertex / edge path behind a table entry ----
// The replay's trace launch: block b replays d_sources[b] once in slot b (nrows <= ws.slots) with
// the early exit on, writes no table row and leaves the slot's vertex records for the walk.
hipError_t launch_heap_replay_trace(const ReplayCSR& g, const ReplayWs& ws,
                                    const uint32_t* d_sources, int nrows,
                                    unsigned long long* d_stats, hipStream_t stream);
// one route's header: the device image of ShdRoute (include/shd_topology_abi.h)
struct TraceRoute {
    int64_t offset;
    int32_t hops, status;
    double latency, reliability;
};
enum { kTraceOk = 0, kTraceUnattached = 1, kTraceBroken = 2, kTraceCap = 3 };
// ids the replay CSR does not carry (uploaded by the first trace): perm (relabelled -> original
// vertex), eid (the igraph_get_eid edge -- lowest id of the parallel group -- of every replay-CSR
// entry), selfEid (lowest-id self loop of every relabelled vertex, -1 = none)
struct TraceIds {
    const int32_t* perm = nullptr;
    const int32_t* eid = nullptr;
    const int32_t* selfEid = nullptr;
};
// eid[j] for every entry of the replay CSR from the parsed edges (document order = edge id)
hipError_t launch_trace_edge_ids(int64_t V, int64_t E, int directed, const int32_t* eu,
                                 const int32_t* ev, const uint32_t* inv, const int32_t* perm,
                                 const uint32_t* rowptr, const uint4* rec, int64_t nadj,
                                 int32_t* eid, hipStream_t stream);
// The requests of one chunk of traced sources, sorted by source: request q has its source's
// records in slot rslot[q], walks from rdst[q] back to rsrc[q] (relabelled ids) and belongs to
// request ridx[q] of the call.
// A chunk that ran the batch kernel's keep launch mixes two chain sources (topo_chain.h): rslot[q]
// is then the source's index i within its chunk and rmap[i] (nmap entries) says where its chains
// are -- the replay slot of a source the replay ran, kNoReplaySlot for a source whose chains are
// the pair records of batch slot i / kf, lane i % kf (PairChains).  rmap == nullptr: every source
// was replayed in slot rslot[q].
constexpr uint32_t kNoReplaySlot = 0xFFFFFFFFu;
struct TraceReqs {
    int64_t n = 0;
    const uint32_t* rslot = nullptr;
    const uint32_t* rsrc = nullptr;
    const uint32_t* rdst = nullptr;
    const uint32_t* ridx = nullptr;
    const uint32_t* rmap = nullptr;
    uint32_t nmap = 0;
};
// the batch slots' pair records after a keep launch of kf sources per batch (SlotWs)
struct PairChains {
    const uint4* prec = nullptr;
    const uint32_t* counters = nullptr;
    int slots = 0, K = 0, kf = 1;
};
// Pass 1: hops and status of every request into routes[ridx]; the entries it needs (hops + 1,
// 0 when not traced) into lneed[q] (chunk order) and gneed[ridx] (request order).
hipError_t launch_route_trace_count(const ReplayCSR& g, const ReplayWs& ws, const TraceReqs& rq,
                                    TraceRoute* routes, int64_t* lneed, int64_t* gneed,
                                    hipStream_t stream);
// Pass 2: vertices and edge ids, source first, at loff[q] of the chunk's staging arrays; latency
// and reliability into routes[ridx].
hipError_t launch_route_trace_write(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                                    const TraceReqs& rq, TraceRoute* routes, const int64_t* loff,
                                    int32_t* stV, int32_t* stE, hipStream_t stream);
// The same two passes over the batch slots' pair records, for the requests whose rmap entry is
// kNoReplaySlot (the replay's passes leave those alone and take the others).  Pass 1 also sets
// broken[i] = 1 (one byte per chunk source, the caller's) for a source with a broken chain.
// Routes of any length: the walk and its staging are in HBM, nothing depends on kMaxHops.
hipError_t launch_route_trace_count_pairs(const ReplayCSR& g, const PairChains& pc,
                                          const TraceReqs& rq, TraceRoute* routes, int64_t* lneed,
                                          int64_t* gneed, uint8_t* broken, hipStream_t stream);
hipError_t launch_route_trace_write_pairs(const ReplayCSR& g, const PairChains& pc,
                                          const TraceIds& ids, const TraceReqs& rq,
                                          TraceRoute* routes, const int64_t* loff, int32_t* stV,
                                          int32_t* stE, hipStream_t stream);
// out[i] = sum of in[0..i) for i < n (device exclusive scan)
hipError_t trace_exclusive_scan(const int64_t* in, int64_t* out, int64_t n, hipStream_t stream);
// offsets of the call: routes[i].offset = goff[i] when the route fits below cap entirely, else
// offset -1 and status kTraceCap (traced routes only)
hipError_t launch_route_trace_place(int64_t n, TraceRoute* routes, const int64_t* goff,
                                    int64_t cap, hipStream_t stream);
// copy the placed routes of a chunk from its staging arrays to outV / outE at their offsets
hipError_t launch_route_trace_scatter(const TraceReqs& rq, const TraceRoute* routes,
                                      const int64_t* loff, const int32_t* stV, const int32_t* stE,
                                      int32_t* outV, int32_t* outE, hipStream_t stream);

// ---- link load (topo_load.hip): per-edge and per-vertex traffic of a set of flows ----
// Accumulators of one call and what the kernels need of the parsed graph.  eload u64[2E]: forward
// half [0, E) (a hop leaves eu[e]; every self loop), reverse half [E, 2E); vload u64[V] in
// relabelled ids (the weight arriving at each vertex).
struct LoadAcc {
    unsigned long long* eload = nullptr;
    unsigned long long* vload = nullptr;
    int64_t E = 0;
    const int32_t* eu = nullptr;  // parsed edge tails (document order = edge id), original ids
};
// counters of one call (u64 words, zeroed by the caller)
enum { LD_ROUTED = 0, LD_BROKEN, LD_HOPW, LD_TREE, LD_COUNT };
// Validate: request q walks rdst -> rsrc with route_trace_kernel<1>'s guards; hops[q] = its hop
// count (self pair: 1), -1 when broken; counts LD_ROUTED / LD_BROKEN and adds w x hops to LD_HOPW.
hipError_t launch_load_validate(const ReplayCSR& g, const ReplayWs& ws, const TraceReqs& rq,
                                const unsigned long long* w, int32_t* hops,
                                unsigned long long* cnt, hipStream_t stream);
// Per-request walk (option "load_walk"): two atomics per hop of every routed request.
hipError_t launch_load_walk(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                            const TraceReqs& rq, const unsigned long long* w,
                            const int32_t* hops, const LoadAcc& acc, hipStream_t stream);
// Validation and per-request walk over the batch slots' pair records (requests whose rmap entry is
// kNoReplaySlot; broken[i] as launch_route_trace_count_pairs).  The tree accumulation below keeps
// its state in the replay slots' vertex-record words, so it has no pair-record form: a call with
// option "load_walk" = 0 replays every source.
hipError_t launch_load_validate_pairs(const ReplayCSR& g, const PairChains& pc, const TraceReqs& rq,
                                      const unsigned long long* w, int32_t* hops,
                                      unsigned long long* cnt, uint8_t* broken,
                                      hipStream_t stream);
hipError_t launch_load_walk_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                  const TraceReqs& rq, const unsigned long long* w,
                                  const int32_t* hops, const LoadAcc& acc, hipStream_t stream);
// Tree accumulation.  The slots' vertex records are reused once the validation is over: the dist
// words become the u64 weight of the vertex's subtree, the heap-position word {bit 31: visited,
// bits 0..30: pending children}; reset clears both for the first nslots slots (the parent slot
// word stays), claim marks the union of the requested chains and counts the children (hops[q]
// becomes -2 for the request that marked its destination: the candidate starter), push carries
// the weights leaf to root, one add per tree vertex into eload / vload.
hipError_t launch_load_reset(const ReplayCSR& g, const ReplayWs& ws, int nslots,
                             hipStream_t stream);
hipError_t launch_load_claim(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                             const TraceReqs& rq, const unsigned long long* w, int32_t* hops,
                             const LoadAcc& acc, unsigned long long* cnt, hipStream_t stream);
hipError_t launch_load_push(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                            const TraceReqs& rq, const int32_t* hops, const LoadAcc& acc,
                            hipStream_t stream);
// out[perm[v]] = vload[v]: relabelled -> original vertex ids
hipError_t launch_load_permute(int64_t V, const int32_t* perm, const unsigned long long* vload,
                               unsigned long long* out, hipStream_t stream);

// ---- link crossings (topo_cross.hip): the flows that cross a set of watched edges / vertices ----
// one crossing: the device image of ShdCrossing (include/shd_topology_abi.h)
struct __attribute__((aligned(16))) CrossRec {
    int32_t flow, watch, hop, reverse;
};
// The watch set of one call: one bit per edge id and per relabelled vertex for the per-hop test;
// on a hit the sorted ids (edges: edge ids; vertices: relabelled ids) are searched for the watch
// index (edges k, vertices ne + k).  wcount / wweight u64[ne + nv]: records and summed flow weight
// of every watch.
struct CrossWatch {
    const uint32_t* ebits = nullptr;
    const uint32_t* vbits = nullptr;
    const int32_t* eids = nullptr;   // ne, ascending
    const int32_t* eidx = nullptr;
    const int32_t* vids = nullptr;   // nv, ascending
    const int32_t* vidx = nullptr;
    int32_t ne = 0, nv = 0;
    int64_t E = 0;
    const int32_t* eu = nullptr;     // parsed edge tails, original ids
    unsigned long long* wcount = nullptr;
    unsigned long long* wweight = nullptr;
};
// counters of one call (u64 words, zeroed by the caller)
enum { CR_RECORDS = 0, CR_FLOWS, CR_COUNT };
// Count: request q (hops[q] from launch_load_validate[_pairs], < 1: no records) walks rdst -> rsrc
// and tests every hop's edge and arrival vertex; its record count into lcnt[q] (chunk order) and
// gcnt[ridx] (request order), the watches' totals into cw.wcount / cw.wweight, the records and the
// flows with one into cnt[CR_RECORDS / CR_FLOWS].
hipError_t launch_cross_count(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                              const TraceReqs& rq, const unsigned long long* w,
                              const int32_t* hops, const CrossWatch& cw, int64_t* lcnt,
                              int64_t* gcnt, unsigned long long* cnt, hipStream_t stream);
// Write: the same walk fills the request's segment [loff[q], loff[q + 1]) of the chunk's staging
// array from its end backwards: route order, within a hop the edge record before the vertex's.
hipError_t launch_cross_write(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                              const TraceReqs& rq, const int32_t* hops, const CrossWatch& cw,
                              const int64_t* loff, CrossRec* stage, hipStream_t stream);
// The same two passes over the batch slots' pair records (requests whose rmap entry is
// kNoReplaySlot).  Without watched edges (cw.ne == 0) no hop's replay-CSR entry is looked up.
hipError_t launch_cross_count_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                    const TraceReqs& rq, const unsigned long long* w,
                                    const int32_t* hops, const CrossWatch& cw, int64_t* lcnt,
                                    int64_t* gcnt, unsigned long long* cnt, hipStream_t stream);
hipError_t launch_cross_write_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                    const TraceReqs& rq, const int32_t* hops, const CrossWatch& cw,
                                    const int64_t* loff, CrossRec* stage, hipStream_t stream);
// copy a chunk's staged records to out at the call's offsets: request q's goff[ridx + 1] -
// goff[ridx] records from stage[loff[q]] to out[goff[ridx]] when they end at or below cap
hipError_t launch_cross_scatter(const TraceReqs& rq, const int64_t* goff, const int64_t* loff,
                                const CrossRec* stage, CrossRec* out, int64_t cap,
                                hipStream_t stream);

// ---- link timeline (topo_timeline.hip): per-time-bin traffic on watched edges / vertices ----
// The bins of one call.  Rows: [0, ne) an edge watch's hops leaving eu[e], [ne, 2 ne) its other
// hops, [2 ne, 2 ne + nv) the vertex watches' arrivals.  acc: u64[rows x nbins], row-major, then
// the `outside` pairs u64[rows x 2] {before t0, at or after the last bin}; zeroed by the caller.
struct TimeBins {
    unsigned long long* acc = nullptr;
    int64_t rows = 0, nbins = 0;
    unsigned long long t0 = 0, binNs = 0;  // ns; binNs > 0 when nbins > 0
};
// counters of one call (u64 words, zeroed by the caller); the hits are IN + BEFORE + AFTER
enum { TL_FLOWS = 0, TL_IN, TL_BEFORE, TL_AFTER, TL_STAGED, TL_COUNT };
// Mark: request q (hops[q] from launch_load_validate[_pairs]) walks rdst -> rsrc until its first
// hit: seg[q] = hops[q] when a hop goes over a watched edge or arrives at a watched vertex, else 0
// (cw.wcount / cw.wweight are not used); the flows with a hit and their hops (self pairs aside:
// they are not staged) into cnt[TL_FLOWS / TL_STAGED].
hipError_t launch_timeline_mark(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                                const TraceReqs& rq, const int32_t* hops, const CrossWatch& cw,
                                int64_t* seg, unsigned long long* cnt, hipStream_t stream);
// Time: a request with a segment [loff[q], loff[q + 1]) of hops[q] entries parks {replay-CSR
// entry, arrival vertex} of its hops there, back to front, then runs front to back: the prefix
// latency by one IEEE add per hop from 0.0, each hit's weight w[q] into the bin of now[q] + ns(the
// prefix before the hop) for an edge watch, + ns(the prefix with it) for a vertex watch; the hit
// counts into cnt[TL_IN / TL_BEFORE / TL_AFTER].
hipError_t launch_timeline_time(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                                const TraceReqs& rq, const unsigned long long* w,
                                const unsigned long long* now, const int32_t* hops,
                                const CrossWatch& cw, const int64_t* loff, uint2* stage,
                                const TimeBins& tb, unsigned long long* cnt, hipStream_t stream);
// The same two passes over the batch slots' pair records (requests whose rmap entry is
// kNoReplaySlot).  Without watched edges (cw.ne == 0) the mark walk looks up no hop's replay-CSR
// entry; the time pass needs it for the hop latency of the flows with a hit.
hipError_t launch_timeline_mark_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                      const TraceReqs& rq, const int32_t* hops,
                                      const CrossWatch& cw, int64_t* seg, unsigned long long* cnt,
                                      hipStream_t stream);
hipError_t launch_timeline_time_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                      const TraceReqs& rq, const unsigned long long* w,
                                      const unsigned long long* now, const int32_t* hops,
                                      const CrossWatch& cw, const int64_t* loff, uint2* stage,
                                      const TimeBins& tb, unsigned long long* cnt,
                                      hipStream_t stream);

// ---- link monitor (topo_monitor.hip): running per-bin link traffic fed by packet windows ----
// one hit of a column pair: the row of TimeBins it lands in and ns(prefix latency), the offset the
// feed adds to a packet's emission time (16 B: one aligned load)
struct __attribute__((aligned(16))) MonRec {
    unsigned long long offNs;
    uint32_t row, pad;
};
// The hit index: pair (s, d) of the A x A column pairs owns rec[off[s A + d], off[s A + d + 1]),
// in hop order, within a hop the edge record before the vertex record; off has A x A + 1 entries.
struct MonIndex {
    const int64_t* off = nullptr;
    const MonRec* rec = nullptr;
    int64_t nrec = 0;
    int32_t A = 0;
};
// counters of a monitor (u64 words): [0, MN_COUNT) cumulative, [MN_COUNT, 2 MN_COUNT) the last
// feed's (zeroed by the caller before it); the hits are IN + BEFORE + AFTER
enum { MN_IN = 0, MN_BEFORE, MN_AFTER, MN_FLOWS, MN_FED, MN_SKIPPED, MN_BAD, MN_COUNT };
// Fill: the timeline's time pass over the requests of one block of sources, request ridx = the
// block's pair: instead of binning, the hits' {ns(prefix), row} are stored at rec[goff[ridx]] ..
// rec[goff[ridx + 1]) (goff: the exclusive scan of launch_cross_count's gcnt); loff / stage as
// launch_timeline_time (the scan of launch_timeline_mark's seg).
hipError_t launch_monitor_fill(const ReplayCSR& g, const ReplayWs& ws, const TraceIds& ids,
                               const TraceReqs& rq, const int32_t* hops, const CrossWatch& cw,
                               const int64_t* loff, uint2* stage, const int64_t* goff, MonRec* rec,
                               hipStream_t stream);
hipError_t launch_monitor_fill_pairs(const ReplayCSR& g, const PairChains& pc, const TraceIds& ids,
                                     const TraceReqs& rq, const int32_t* hops,
                                     const CrossWatch& cw, const int64_t* loff, uint2* stage,
                                     const int64_t* goff, MonRec* rec, hipStream_t stream);
// out[i] = in[i] + base for i < n
hipError_t launch_monitor_offsets(const int64_t* in, int64_t* out, int64_t n, int64_t base,
                                  hipStream_t stream);
// Feed: packet k (skipped when delivered[k] == 0; counted MN_BAD, nothing read through it, when a
// column is outside [0, A)) adds its weight (payload[k], NULL: 1) for every record of its pair to
// the bin of now[k] + offNs (NULL: 0), by TimelineOut::add's rule.  Enqueued, not awaited.
hipError_t launch_monitor_feed(int64_t n, const int32_t* src, const int32_t* dst,
                               const uint32_t* payload, const unsigned long long* now,
                               const uint8_t* delivered, const MonIndex& ix, const TimeBins& tb,
                               unsigned long long* cnt, hipStream_t stream);
// the same with u64 weights (the host feeds)
hipError_t launch_monitor_feed_u64(int64_t n, const int32_t* src, const int32_t* dst,
                                   const unsigned long long* weight, const unsigned long long* now,
                                   const uint8_t* delivered, const MonIndex& ix, const TimeBins& tb,
                                   unsigned long long* cnt, hipStream_t stream);

// ---- traffic matrix (topo_matrix.hip): packet windows summed into per-pair cells ----
// one cell of the M x M matrix (row = source, column = destination): the two sums of a packet's
// adds share a line, the export loads 16 B per cell
struct __attribute__((aligned(16))) MatCell {
    unsigned long long packets, weight;
};
// one reported cell: the device image of ShdMatrixFlow (include/shd_topology_abi.h), 32 B
struct __attribute__((aligned(16))) MatFlowRec {
    int32_t srcVertex, dstVertex, srcIndex, dstIndex;
    unsigned long long packets, weight;
};
// counters of a matrix (u64 words): [0, MX_COUNT) cumulative, [MX_COUNT, 2 MX_COUNT) the last
// feed's (zeroed by the caller before it)
enum { MX_FED = 0, MX_SKIPPED, MX_BAD, MX_COUNT };
// the u64 totals of one read's count pass (zeroed by the caller)
enum {
    MT_CELLS = 0, MT_PACKETS, MT_WEIGHT, MT_SELF_CELLS, MT_SELF_PACKETS, MT_SELF_WEIGHT,
    MT_ACTIVE_SRC, MT_COUNT
};
// Feed: packet k (skipped when delivered[k] == 0; counted MX_BAD, nothing read through it, when a
// column is outside [0, A) or colMap holds no index in [0, M) for it) adds 1 and its weight
// (payload[k], NULL: 1) to cell (colMap[src[k]], colMap[dst[k]]).  Enqueued, not awaited.
hipError_t launch_matrix_feed(int64_t n, const int32_t* src, const int32_t* dst,
                              const uint32_t* payload, const uint8_t* delivered,
                              const int32_t* colMap, int32_t A, MatCell* cells, int32_t M,
                              unsigned long long* cnt, hipStream_t stream);
// the same with u64 weights (the host feeds)
hipError_t launch_matrix_feed_u64(int64_t n, const int32_t* src, const int32_t* dst,
                                  const unsigned long long* weight, const uint8_t* delivered,
                                  const int32_t* colMap, int32_t A, MatCell* cells, int32_t M,
                                  unsigned long long* cnt, hipStream_t stream);
// Re-layout: old cell (i, j) of the M0 x M0 matrix goes to (map[i], map[j]) of the M1 x M1 one
// (map: i32[M0], strictly ascending, every entry in [0, M1)); the new cells are zeroed first.
hipError_t launch_matrix_relayout(const MatCell* old, int32_t M0, const int32_t* map,
                                  MatCell* cells, int32_t M1, hipStream_t stream);
// cells[k] += add[k] for k < n (the uploaded host cells of a read)
hipError_t launch_matrix_add(MatCell* cells, const MatCell* add, int64_t n, hipStream_t stream);
// Count: one workgroup per row i: rowCells[i] = its reported cells (packets != 0 || weight != 0),
// sentP / sentW [i] = its sums over all cells, rowPeakW / rowPeakCell [i] = the largest weight of
// a reported cell and the lowest i M + j reaching it (0 / -1: none); recvP / recvW [j] += the
// reported cells of column j, colActive[j] = 1 for a column with one (u64[M] / u32[M], zeroed by
// the caller); tot: the MT_ totals.
struct MatCount {
    int64_t* rowCells = nullptr;
    unsigned long long* sentP = nullptr;
    unsigned long long* sentW = nullptr;
    unsigned long long* recvP = nullptr;
    unsigned long long* recvW = nullptr;
    uint32_t* colActive = nullptr;
    unsigned long long* rowPeakW = nullptr;
    int64_t* rowPeakCell = nullptr;
    unsigned long long* tot = nullptr;
};
hipError_t launch_matrix_count(const MatCell* cells, int32_t M, const MatCount& o,
                               hipStream_t stream);
// Fill: row i writes its reported cells' records, columns ascending, at out[rowOff[i]] .. (rowOff:
// the exclusive scan of rowCells); records at or past cap are not written.  mv: i32[M].
hipError_t launch_matrix_fill(const MatCell* cells, int32_t M, const int32_t* mv,
                              const int64_t* rowCells, const int64_t* rowOff, MatFlowRec* out,
                              int64_t cap, hipStream_t stream);

// ---- table diff (topo_diff.hip): the changed pairs of two A x A tables ----
// one changed pair: the device image of ShdTableChange (include/shd_topology_abi.h); hops =
// hops0 | hops1 << 16
struct __attribute__((aligned(16))) DiffRec {
    int32_t srcCol, dstCol;
    double lat0, lat1, rel0, rel1;
    uint32_t hops, kind;
};
enum : uint32_t { kDiffLatRose = 1, kDiffLatFell = 2, kDiffRel = 4, kDiffHops = 8 };
// the two tables of one call, row-major A x A, on the current device
struct DiffTables {
    const double2* lr0 = nullptr;
    const double2* lr1 = nullptr;
    const uint16_t* hops0 = nullptr;
    const uint16_t* hops1 = nullptr;
    int32_t A = 0;
};
// Count: one workgroup per row s: rowChanged[s] = its changed pairs, rowWorstRise[s] /
// rowWorstCol[s] = its largest lat1 - lat0 and the lowest column reaching it (0.0 / -1 when no
// latency rises), kindCount[i] += its pairs with kind bit 1 << i (u64[4], zeroed by the caller).
hipError_t launch_diff_count(const DiffTables& t, int64_t* rowChanged, double* rowWorstRise,
                             int32_t* rowWorstCol, unsigned long long* kindCount,
                             hipStream_t stream);
// Fill: row s writes its changed pairs' records, columns ascending, at out[rowOff[s]] .. (rowOff:
// the exclusive scan of rowChanged); records at or past cap are not written.
hipError_t launch_diff_fill(const DiffTables& t, const int64_t* rowChanged, const int64_t* rowOff,
                            DiffRec* out, int64_t cap, hipStream_t stream);

// ---- flow impact (topo_impact.hip): the changed flows of a set of column pairs ----
// one changed flow: the device image of ShdFlowChange (include/shd_topology_abi.h); hops =
// hops0 | hops1 << 16
struct __attribute__((aligned(16))) ImpactRec {
    int64_t flow;
    double lat0, lat1, rel0, rel1;
    uint32_t hops, kind;
};
// the u64 totals of one call (zeroed by the caller)
enum {
    IT_COMPARED = 0, IT_UNATTACHED, IT_CHANGED, IT_KIND_COUNT,  // (4 kind bits)
    IT_WEIGHT = IT_KIND_COUNT + 4, IT_CHANGED_WEIGHT, IT_KIND_WEIGHT,
    IT_DELAY_RISE = IT_KIND_WEIGHT + 4, IT_DELAY_FALL, IT_HOPS_RISE, IT_HOPS_FALL,
    IT_COUNT
};
constexpr int kImpactMaxEdges = 1024;
// the fill pass's count of the words it gathered for: kImpactShards counters, each on a 64-B line
// of its own (one counter for every wavefront's add would serialise the pass on that address)
constexpr int kImpactShards = 64, kImpactShardStride = 8;
// The flows of one call and what the count pass writes.  Tile blk = flows [blk T, (blk + 1) T),
// T = impact_tile_flows(); words has T / 64 words per tile, word k / 64 = the changed flows of
// [64 (k / 64), + 64) (every word of every tile is written); tileChanged / tileRise / tileFlow have
// one entry per tile: its changed flows, its largest lat1 - lat0 over the flows whose latency rose
// and the lowest flow reaching it (0.0 / -1: none).  hist = u64[2 (nb + 1)], counts then weights;
// srcW / dstW = u64[A] or NULL.
struct ImpactFlows {
    const int32_t* src = nullptr;
    const int32_t* dst = nullptr;
    int64_t n = 0;
    const unsigned long long* edges = nullptr;
    int32_t nb = 0;
};
struct ImpactOut {
    unsigned long long* words = nullptr;
    int64_t* tileChanged = nullptr;
    double* tileRise = nullptr;
    int64_t* tileFlow = nullptr;
    unsigned long long* tot = nullptr;
    unsigned long long* hist = nullptr;
    unsigned long long* srcW = nullptr;
    unsigned long long* dstW = nullptr;
};
int64_t impact_tile_flows();
// Count: the weights are w64 (the host variant), else w32 (a packet window's payload), else 1.
hipError_t launch_impact_count(const DiffTables& t, const ImpactFlows& f,
                               const unsigned long long* w64, const uint32_t* w32,
                               const ImpactOut& o, hipStream_t stream);
// Fill: the changed flows' records at out[tileOff[blk] + rank in the tile] (tileOff: the
// exclusive scan of tileChanged); records at or past cap are not written.  gathered (u64
// [kImpactShards x kImpactShardStride], zeroed by the caller): the words gathered for, summed
// over the shards.
hipError_t launch_impact_fill(const DiffTables& t, const ImpactFlows& f,
                              const unsigned long long* words, const int64_t* tileChanged,
                              const int64_t* tileOff, ImpactRec* out, int64_t cap,
                              unsigned long long* gathered, hipStream_t stream);

// ---- load shift (topo_shift.hip): the entries whose load differs between two link loads ----
// one changed entry: the device image of ShdLoadChange (include/shd_topology_abi.h)
struct __attribute__((aligned(16))) ShiftRec {
    int32_t kind, id, idA, idB;
    unsigned long long before, after;
};
// the u64 totals of one call (zeroed by the caller): five counts and two weighted sums by kind
// (forward half, reverse half, vertex), then the two sums over the halves one side lacks
enum {
    SH_CHANGED = 0, SH_GAINED = 3, SH_LOST = 6, SH_NEW = 9, SH_ABANDONED = 12, SH_GAINED_W = 15,
    SH_LOST_W = 18, SH_DISPLACED = 21, SH_APPEARED, SH_COUNT
};
// the {largest value, lowest entry reaching it} pairs of one call
enum { SP_GAIN = 0, SP_LOSS, SP_PEAK_BEFORE, SP_PEAK_AFTER, SP_COUNT };
// One side of the comparison: a link load's sums on the device -- eload u64 [2 E] by the side's own
// edge ids (forward halves, then reverse halves), vload u64 [V] by original vertex id -- and its
// place in the root's numbering: gaps = the root edge ids the side lacks, strictly ascending,
// ngaps = R - E of them (none: a root topology).  Root edge r is the side's edge r - (the number
// of gaps below r), or no edge of it when r is a gap.
struct ShiftSide {
    const unsigned long long* eload = nullptr;
    const unsigned long long* vload = nullptr;
    const int32_t* gaps = nullptr;
    int32_t ngaps = 0;
    int64_t E = 0;
};
// The entries x in [0, 2 R + V) of one call -- forward halves, reverse halves, vertices -- and what
// the count pass writes.  Tile blk = entries [blk T, (blk + 1) T), T = shift_tile_entries(); words
// has T / 64 words per tile (every word of every tile is written); tileChanged has one entry per
// tile; tileVal / tileIdx have SP_COUNT per tile: the tile's pairs (0 / -1: none).
struct ShiftIn {
    ShiftSide a, b;
    int64_t R = 0, V = 0;
};
struct ShiftOut {
    unsigned long long* words = nullptr;
    int64_t* tileChanged = nullptr;
    unsigned long long* tileVal = nullptr;
    int64_t* tileIdx = nullptr;
    unsigned long long* tot = nullptr;
};
int64_t shift_tile_entries();
hipError_t launch_shift_count(const ShiftIn& in, const ShiftOut& o, hipStream_t stream);
// the call's pairs from the tiles': pairVal u64 [SP_COUNT], pairIdx i64 [SP_COUNT]
hipError_t launch_shift_reduce(int64_t tiles, const unsigned long long* tileVal,
                               const int64_t* tileIdx, unsigned long long* pairVal,
                               int64_t* pairIdx, hipStream_t stream);
// Fill: the changed entries' records at out[tileOff[blk] + rank in the tile] (tileOff: the
// exclusive scan of tileChanged); records at or past cap are not written.  gathered: as
// launch_impact_fill's.
hipError_t launch_shift_fill(const ShiftIn& in, const unsigned long long* words,
                             const int64_t* tileChanged, const int64_t* tileOff, ShiftRec* out,
                             int64_t cap, unsigned long long* gathered, hipStream_t stream);

hipError_t launch_pair_table_complete(int A, int64_t row0, int64_t rows, const double* elatAA,
                                      const double* elossAA, const double* vlossA, double2* out_lr,
                                      uint16_t* out_hops, double* out_rowmin,
                                      unsigned long long* d_stats, hipStream_t stream);

hipError_t launch_packet_route(int64_t n, const int32_t* src, const int32_t* dst,
                               const uint32_t* payload, const uint32_t* state_in,
                               const uint64_t* now, const double2* table, int64_t A,
                               uint64_t jump, int clamp, uint64_t* t_out, uint32_t* state_out,
                               uint8_t* delivered, unsigned long long* d_bad, hipStream_t stream);

// ---- route schedule (topo_schedule.hip): each packet routed by the table live at its emit time ----
// The k tables (A x A each, on the current device) and their start times, passed to the kernel by
// value: wave-uniform, so they arrive in SGPRs.  from[0] = 0, from strictly ascending; entries at
// and past k are not read.
constexpr int kScheduleMax = 16;
struct ScheduleTables {
    const double2* lr[kScheduleMax] = {};
    unsigned long long from[kScheduleMax] = {};
    int32_t k = 0;
};
// launch_packet_route with the table of epoch e(i) = the largest e with from[e] <= now[i] for
// packet i; epoch (nullable) receives e(i), one byte per packet; cnt (u64 [k][3], zeroed by the
// caller): {packets, delivered, columns outside [0, A)} of every epoch.  Enqueued, not awaited.
hipError_t launch_route_schedule(const ScheduleTables& t, int64_t n, const int32_t* src,
                                 const int32_t* dst, const uint32_t* payload,
                                 const uint32_t* state_in, const uint64_t* now, int64_t A,
                                 uint64_t jump, int clamp, uint64_t* t_out, uint32_t* state_out,
                                 uint8_t* delivered, uint8_t* epoch, unsigned long long* cnt,
                                 hipStream_t stream);

hipError_t launch_row_min(int64_t rows, int64_t A, const double2* lr, double* out_rowmin,
                          hipStream_t stream);

hipError_t launch_fill_u64(unsigned long long* p, unsigned long long v, int64_t n,
                           hipStream_t stream);
// p[b * stride + i] = v for b < nb, i < n
hipError_t launch_fill_u64_strided(unsigned long long* p, unsigned long long v, int64_t nb,
                                   int64_t stride, int64_t n, hipStream_t stream);

// ---- graph preparation on the GPU (topo_prep.hip), once per topology: DESIGN.md 3.1 ----
// Input arrays are the parsed graph in HBM (document order: eu / ev int32[E], elat / eloss f64[E],
// vloss f64[V]); outputs are in the relabelled vertex order.  Each call synchronises `st`.
// degrees of the non-loop graph (deg u32[V], in + out when directed), the lowest-id self loop
// (selfE, ~0 = none) and *nadj = 2 x non-loop edges
hipError_t prep_degrees(int64_t V, int64_t E, const int32_t* eu, const int32_t* ev, uint32_t* deg,
                        uint32_t* selfE, int64_t* nadj, hipStream_t st);
// relabel (degree descending, the tail grouped by its primary hub among the first H): perm
// (new -> old), inv (old -> new), rowptr u32[V+1], per-vertex loss and self-loop arrays
hipError_t prep_relabel(int64_t V, int64_t E, uint32_t H, const int32_t* eu, const int32_t* ev,
                        const uint32_t* deg, const uint32_t* selfE, const double* elat,
                        const double* eloss, const double* vloss_in, uint32_t* perm,
                        uint32_t* inv, uint32_t* rowptr, double* vloss, double* selfLat,
                        double* selfLoss, hipStream_t st);
// 16-B adjacency records {col, 0, f64 w} rows ascending by (neighbour, edge id), and aloss
// (nullable).  mode 0: every non-loop edge in both rows (undirected, nadj = 2E'); 1: out-rows
// only, 2: in-rows only (directed, nadj = E'); for modes 1 and 2 rowptr (u32[V+1]) is counted
// from the entries
enum { kAdjBoth = 0, kAdjOut = 1, kAdjIn = 2 };
hipError_t prep_adjacency(int64_t V, int64_t E, int64_t nadj, const int32_t* eu, const int32_t* ev,
                          const uint32_t* inv, const double* elat, const double* eloss,
                          uint32_t* adj, double* aloss, hipStream_t st, int mode = kAdjBoth,
                          uint32_t* rowptr = nullptr);
// pi = d(h0, .) from vertex 0 (f64[V], +inf = unreached); *iterations = frontier rounds
hipError_t prep_h0_distances(int64_t V, const uint32_t* rowptr, const uint32_t* adj, double* pot,
                             int* iterations, hipStream_t st);
// h0 tree (sptPar u32[V], spt {parent, slot in v's row, f64 w, f64 loss, pad} 32 B [V]), the
// records' pi / kappa0 field, *piMax = the largest finite pi; hub rows by segments (hs).
// what: kTreeParents (the tree, from rows of candidate parents: in-rows when directed) |
// kTreeKappa (kappa0 and the records' field, from relaxation rows: out-rows when directed)
enum { kTreeParents = 1, kTreeKappa = 2 };
hipError_t prep_tree(int64_t V, int64_t nadj, const HubSegs& hs, const uint32_t* rowptr,
                     uint32_t* adj, const double* aloss, const double* pot, uint32_t* sptPar,
                     uint32_t* spt, double* piMax, hipStream_t st,
                     int what = kTreeParents | kTreeKappa);
// the plain kappa-sorted relaxation copy (adjk, kap, ksum, kap0) of adj: also restores it after
// a target-aware re-sort when the target-aware order no longer applies
hipError_t launch_kappa_copy(int64_t V, int64_t nadj, const HubSegs& hs, const uint32_t* rowptr,
                             const uint32_t* adj, const double* pot, const uint32_t* sptPar,
                             uint32_t* adjk, float* kap, float* ksum, float* kap0,
                             hipStream_t st);

// the heap replay's incidence CSR (ReplayCSR) from the parsed edges in HBM: rows in relabelled
// ids, each in igraph_incident order (ascending original neighbour; parallel groups merged, the
// lowest edge id's latency / loss for the hop, the group's minimum latency for the heap).
// rec / own / hop hold up to 2E (E directed) entries; *nrec = the entries written.
hipError_t prep_replay_csr(int64_t V, int64_t E, int directed, const int32_t* eu,
                           const int32_t* ev, const double* elat, const double* eloss,
                           const uint32_t* inv, const double* pot, uint32_t* rowptr, uint4* rec,
                           uint32_t* own, double2* hop, int64_t* nrec, hipStream_t st);

// Load each kernel module's code object now (dev_init) instead of at its first launch inside
// the first build: the runtime loads code objects lazily.
hipError_t preload_batch_module();
hipError_t preload_prep_module();
hipError_t preload_kernels_module();
hipError_t preload_replay_module();

}  // namespace shdtopo
