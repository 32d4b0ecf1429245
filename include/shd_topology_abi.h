/*
 * shd_topology_abi.h -- C ABI of libshdtopo.so, the MI355X-native routing engine that replaces
 * Shadow's topology subsystem (src/topology/shd-topology.c + shd-path.c, Shadow v1.11.1).
 *
 * Part 1 is exactly the reference header src/topology/shd-topology.h:12-22 with the GLib
 * typedefs written as plain C (gchar=char, gboolean=int, gdouble=double, guint64=uint64_t), so
 * Shadow's callers link against it unchanged:
 *   runnable/action/shd-load-topology.c:50,79  topology_new
 *   engine/shd-slave.c:147                     topology_free
 *   host/shd-host.c:97 / :172 / :1082          topology_attach / topology_detach / isRoutable
 *   engine/shd-worker.c:352,360                topology_getReliability / topology_getLatency
 *   engine/shd-slave.c:261-268                 topology_getLatency (TCP autotune)
 *
 * Imports resolved from the Shadow executable at load time (weak: a standalone process loads
 * libshdtopo_shim.so, a restatement of these four functions, first):
 *   uint32_t address_toNetworkIP(Address*)       src/topology/shd-address.c:114
 *   double   random_nextDouble(Random*)          src/utility/shd-random.c:34
 *   void     worker_updateMinTimeJump(double)    src/engine/shd-worker.c:459
 *
 * Part 2 adds the two entry points the north star names: the global minimum
 * latency (absent in the reference: it is pushed from shd-topology.c:500-511, K2) and the
 * per-window packet batch (engine-side adapter of src/engine/shd-worker.c:332-370).
 *
 * Part 3 is the device-level boundary used by multi-GPU drivers (one process per GPU): shard
 * rows into caller-owned HBM buffers, install an all-gathered table, route packets already
 * resident in HBM.  Device pointers are plain `void*` / typed pointers into HBM; `stream` is a
 * hipStream_t passed as void* (NULL = the library's own stream).  No torch types anywhere.
 *
 * Errors follow the reference: getters return -1.0 for an unattached address
 * (shd-topology.c:882-892, logs "critical"); an attached-but-unroutable pair is a fatal
 * error() in the reference (shd-topology.c:917-928) -- here it aborts too unless the
 * "abort_on_error" option is set to 0, in which case the getter returns -1.0.
 */
#ifndef SHD_TOPOLOGY_ABI_H_
#define SHD_TOPOLOGY_ABI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct _Topology Topology;
typedef struct _Address Address; /* Shadow's, opaque here */
typedef struct _Random Random;   /* Shadow's, opaque here */

/* ---------------- Part 1: src/topology/shd-topology.h:14-22 ---------------- */
/* shd-topology.c:1237  NULL on failure (parse error, not strongly connected, latency <= 0) */
Topology* topology_new(const char* graphPath);
/* shd-topology.c:1199 */
void topology_free(Topology* top);
/* shd-topology.c:1154  consumes exactly one random_nextDouble(randomSourcePool) unless LPM */
void topology_attach(Topology* top, Address* address, Random* randomSourcePool, char* ipHint,
                     char* geocodeHint, char* typeHint, uint64_t* bwDownOut, uint64_t* bwUpOut);
/* shd-topology.c:1190 */
void topology_detach(Topology* top, Address* address);
/* shd-topology.c:960 */
int topology_isRoutable(Topology* top, Address* srcAddress, Address* dstAddress);
/* shd-topology.c:940  ms, -1.0 on failure */
double topology_getLatency(Topology* top, Address* srcAddress, Address* dstAddress);
/* shd-topology.c:950  [0,1], -1.0 on failure */
double topology_getReliability(Topology* top, Address* srcAddress, Address* dstAddress);

/* ---------------- Part 2: north-star additions ---------------- */
/* Global min latency (ms) over all attached pairs incl. self pairs; replaces the lazily
 * pushed minimum of shd-topology.c:500-511.  Builds the table if needed.  -1.0 on failure. */
double topology_getMinimumLatency(Topology* top);

typedef struct {
    uint32_t srcIP;         /* network order, as address_toNetworkIP */
    uint32_t dstIP;
    uint32_t payloadLength; /* packet_getPayloadLength: 0 = control packet, never dropped */
    uint32_t rngState;      /* sender host's rand_r state BEFORE the draw */
    uint64_t now;           /* worker clock at emit, ns */
} TopoPacketIn;

typedef struct {
    uint64_t time;          /* delivery event time, ns (0 if dropped) */
    uint32_t rngState;      /* sender's rand_r state after the draw */
    uint8_t delivered;      /* PDS_INET_SENT (1) / PDS_INET_DROPPED (0) */
    uint8_t _pad[3];
} TopoPacketOut;

/* worker_schedulePacket (shd-worker.c:332-370) for n packets of one scheduler window, host
 * buffers (includes the PCIe copies).  jumpNs/clampInterHost: shd-worker.c:310-324.  In lazy
 * mode every packet is answered as the reference's getReliability/getLatency calls would have
 * been in array (= emission) order: first-rooted-wins orientation and running-minimum pushes.
 * The caller captures in[i].rngState before the sender's draw and advances the sender's
 * Random by that one draw itself (tests/c/engine_window.c shows the engine-side adapter).
 * A packet whose address is not attached is not routed (the reference's getters return -1.0
 * for it, shd-topology.c:882-892): delivered 0, time 0, rngState after its draw; the others are
 * routed.  Returns 0 when every packet was routed, else the number of packets that were not, or
 * a negative error (the outputs are then undefined). */
int topology_routePacketBatch(Topology* top, const TopoPacketIn* in, TopoPacketOut* out, size_t n,
                              uint64_t jumpNs, int clampInterHost);

/* ---------------- Part 3: device-level boundary / library extras ---------------- */
int shdtopo_version(void);
/* CDATA topologies (shd-load-topology.c:57-82) without the temp file */
Topology* shdtopo_new_from_buffer(const char* graphml, size_t len);

/* options: "abort_on_error" (1), "lazy" (1 = K3 first-rooted-wins emulation, 0 = eager
 * forward rows), "delta" (delta-stepping bucket width, ms; default the mean edge latency),
 * "h0_phase" (where the landmark h0 sits in its bucket, [0, 1); default: at its bucket's end, a
 * gap of min(1 % of delta, half the smallest edge latency) below it; < 0: the round-4 bucket
 * shifts), "slots" (concurrent SSSP
 * workgroups), "device" (HIP device ordinal), "lds_hubs" (cap on LDS-resident hub distances,
 * -1 = fill), "par_hubs" (hubs with SSSP parent hints), "row_scan_chunk" (parent-pass pairs
 * per row-scan chunk, 64..2^20, default 16384: 16 B x batch of workspace per pair), "wg_per_cu" (SSSP workgroups sharing a
 * CU's LDS), "far_cap" / "near_cap" (entries per window bucket and overflow pile / per near
 * queue, 0 = sized from V; small values force the scanning fallback), "events" (1 = diagnostic
 * kernel with event counters), "tie_replay" (1: rows whose target chains cross a d-tied parent
 * are recomputed by the exact heap replay; 0: reported only), "replay_all" (test hook: every row
 * through the replay), "replay_slots" (concurrent replay wavefronts, 0 = auto), "replay_landmark"
 * (1: the replay skips relaxations into vertices a landmark bound proves popped),
 * "replay_int_keys" (1: u32 heap keys when every latency is an integer and V x max latency
 * < 2^32 - 1 -- exact; 0: always f64 keys), "tie_dense"
 * (-1 auto / 0 / 1: every row through the replay, no batch kernel, once a build replayed >= 90 %
 * of its rows or, on integer latencies, a 64-row probe before the first batched build found
 * >= 90 % of its rows crossing a tie), "devices" (N:
 * the table is built by N GPUs of this process -- rows sharded, RCCL all-gather of the rows and
 * all-reduce(MIN) of the minimum; devices device..device+N-1), "rccl" (1: use that exchange even
 * with one device), "batch" (sources per SSSP workgroup: 8; 2 / 4 / 16; any other value is
 * rejected), "batch_fill" (sources per batch, <= batch; 0 = auto: the fewest that finish the rows
 * in the same rounds of the slots), "source_order" / "batch_order" (row grouping and batch
 * dequeue order), "target_skip" (1: the batch relaxation drops pairs into
 * non-target vertices that would relax nothing reaching a target), "target_kappa" (iterations of
 * the target-aware kappa fixpoint behind that test, 0 = the row's smallest kappa; default 6),
 * "share" (1: a batched launch's workgroups that run out of batches take part in the running
 * batches' parent walks and epilogues -- the help board; 0, the default: each batch stays in its
 * workgroup and the board-less kernel runs; -1: the board for a launch whose batches fit one
 * round of the slots), "balance" (1, the default: from the second batched build of a graph on,
 * batches are sized (one round of the slots) or dequeued longest first (several rounds) by the
 * sources' costs measured from the earlier builds' batch times; 0: the grouping order only),
 * "trace_chunk" (sources per replay launch of shdtopo_trace_routes; 0, the default: the replay's
 * wavefront slots; a small value forces several chunks -- a test hook; it bounds
 * shdtopo_link_load's launches too), "load_walk" (shdtopo_link_load: 1, the default, walks every
 * request's route with two atomics per hop; 0 sums the weights leaf to root over each source's
 * tree of requested routes, one add per tree vertex -- measured no faster at the bench size,
 * DESIGN.md 3.7; both give the same sums; any other value is rejected), "trace_batch"
 * (shdtopo_trace_routes / shdtopo_link_load: 1, the default, takes a source's routes from the
 * batch kernel's parent records where that is exact and replays only the other sources; 0 always
 * runs the heap replay -- the A/B and test baseline; both give the same bytes; any other value is
 * rejected), "h0_seed" (1, the default: the batch kernel's landmark bound d_j(h0) of source j
 * starts at the graph preparation's d(s_j, h0), scaled up by max(1e-9, 4 V 2^-53), instead of
 * +inf, so the landmark filter, the target skip and the kappa cut prune from the first expansion;
 * 0: the bound is learnt from the kernel's tentative value of h0 alone; both give the same table),
 * "matrix_mb" (the bytes a traffic matrix's cells may take, a double in MB; 0, the default: half
 * of the device memory free when the matrix grows, no cap for host cells; a negative value is
 * rejected).
 * Returns 0 or -1 for an unknown key / bad value. */
int shdtopo_set_option(Topology* top, const char* key, double value);

/* attach by raw IP and a rand_r state (same algorithm and RNG use as topology_attach) */
int32_t shdtopo_attach_ip(Topology* top, uint32_t ip, uint32_t* rngState, const char* ipHint,
                          const char* geocodeHint, const char* typeHint, uint64_t* bwDownOut,
                          uint64_t* bwUpOut);
/* topology_detach by raw IP (shd-topology.c:1190-1197: the mapping goes, cached paths stay) */
void shdtopo_detach_ip(Topology* top, uint32_t ip);
double shdtopo_get_latency_ip(Topology* top, uint32_t srcIP, uint32_t dstIP);
double shdtopo_get_reliability_ip(Topology* top, uint32_t srcIP, uint32_t dstIP);

/* graph facts */
int64_t shdtopo_num_vertices(Topology* top);
int64_t shdtopo_num_edges(Topology* top);
int shdtopo_is_complete(Topology* top);
int shdtopo_is_directed(Topology* top);

/* attached-vertex table geometry: A distinct attached vertices, ascending vertex index */
int64_t shdtopo_num_attached(Topology* top);
int64_t shdtopo_attached_vertices(Topology* top, int32_t* out, int64_t cap);
int32_t shdtopo_column_of_ip(Topology* top, uint32_t ip);          /* -1 if unattached */
int32_t shdtopo_vertex_of_ip(Topology* top, uint32_t ip);          /* -1 if unattached */

/* Build the whole A x A table on this process's GPU(s) (SSSP or complete-pair kernel). */
int shdtopo_build(Topology* top);
/* Row shard [*r0, *r1) of device d out of n for A rows: ceil(A / n) rows each, the last shards
 * possibly short or empty (the split of option "devices" and of shadow_amd.sharding). */
void shdtopo_shard_rows(int64_t A, int n, int d, int64_t* r0, int64_t* r1);
/* Build rows [row0,row1) into caller-owned HBM: lr = {f64 lat, f64 rel}[rows][A],
 * hops = u16[rows][A], rowmin = f64[rows] (may be NULL).  Enqueued on `stream`. */
int shdtopo_build_rows(Topology* top, int64_t row0, int64_t row1, void* d_lr, void* d_hops,
                       void* d_rowmin, void* stream);
/* Install an assembled A x A table (e.g. after an RCCL all-gather) as the routing table.
 * The library copies it into its own buffers (same device). */
int shdtopo_bind_table(Topology* top, const void* d_lr, const void* d_hops, double globalMin,
                       void* stream);
/* Install an assembled table in place: the library reads the caller's buffers (same device; they
 * must stay valid and unchanged until the next build or bind) instead of copying 1.8 GB. */
int shdtopo_bind_table_ref(Topology* top, const void* d_lr, const void* d_hops, double globalMin,
                           void* stream);
/* Rebuild the whole table now for the current attached set (topology_getLatency & co. build it
 * lazily; this forces the build, e.g. to time it). */
int shdtopo_rebuild(Topology* top);
/* Copy the current table to host memory (lat, rel: f64[A*A]; hops: u16[A*A]; any may be NULL) */
int shdtopo_table_to_host(Topology* top, double* lat, double* rel, uint16_t* hops);

/* topology_routePacketBatch with the packets' vertices instead of their IPs (SoA host arrays;
 * -1 = not attached): the window adapter resolves them at emit, so a host detached before the
 * flush (the reference routed its packet at emit, shd-worker.c:345-369) is still routed while its
 * vertex is a table column.  Same outputs and return value. */
int shdtopo_route_batch_vertices(Topology* top, const int32_t* srcVertex, const int32_t* dstVertex,
                                 const uint32_t* payloadLength, const uint32_t* rngState,
                                 const uint64_t* now, size_t n, uint64_t jumpNs,
                                 int clampInterHost, TopoPacketOut* out);
/* Window bookkeeping of the engine-side adapter (include/shd_topology_window.h): while at least
 * one window is registered (hold +1 at topowindow_new, -1 at topowindow_free), a vertex that
 * loses its last host keeps its table column until shdtopo_window_release (called by every
 * flush after it routed), so the packets it emitted in the window are routed as the reference
 * routed them at emit.  Returns 0, -1 on a NULL topology. */
int shdtopo_window_hold(Topology* top, int delta);
int shdtopo_window_release(Topology* top);

/* Route n packets whose inputs are resident in HBM (SoA, attached-column indices). */
int shdtopo_route_batch_device(Topology* top, const int32_t* d_srcCol, const int32_t* d_dstCol,
                               const uint32_t* d_payload, const uint32_t* d_stateIn,
                               const uint64_t* d_now, int64_t n, uint64_t jumpNs, int clamp,
                               uint64_t* d_time, uint32_t* d_stateOut, uint8_t* d_delivered,
                               void* stream);

/* The same on device slot `slot` of a multi-GPU Topology (option "devices": every slot holds the
 * whole table after the exchange; inputs and outputs in that device's HBM, stream NULL = the
 * slot's own).  Slot 0 = shdtopo_route_batch_device. */
int shdtopo_route_batch_device_slot(Topology* top, int slot, const int32_t* d_srcCol,
                                    const int32_t* d_dstCol, const uint32_t* d_payload,
                                    const uint32_t* d_stateIn, const uint64_t* d_now, int64_t n,
                                    uint64_t jumpNs, int clamp, uint64_t* d_time,
                                    uint32_t* d_stateOut, uint8_t* d_delivered, void* stream);

/* lazily tracked minimum (reference trajectory, shd-topology.c:500-511) */
double shdtopo_get_lazy_minimum_latency(Topology* top);

/* Test hook: the source rows the lazy emulation has materialised so far (the rows whose
 * computeSourcePaths the reference would have run, shd-topology.c:900-915): up to cap vertices
 * with, per vertex, the attach epoch of its latest materialisation (epochs grow; a row
 * materialised again after a late attach gets a larger one) and the row minimum that
 * materialisation offered to the running minimum (shd-topology.c:500-511).  Any array may be
 * NULL.  Returns the number of materialised rows (may exceed cap), -1 on a NULL topology. */
int64_t shdtopo_lazy_rows(Topology* top, int32_t* vertex, uint64_t* epoch, double* rowmin,
                          int64_t cap);

typedef struct {
    double build_ms;          /* wall time of the last table build (device, event timed) */
    double sssp_kernel_ms;    /* event-timed duration of the last SSSP / pair kernel launch */
    double route_kernel_ms;   /* event-timed duration of the last packet-route launch */
    int64_t sources;          /* rows computed by the last build */
    int64_t targets;          /* A */
    int64_t ambiguous_pairs;  /* pairs whose path crosses a d-tied parent (heap order decides) */
    int64_t relaxations;      /* edge relaxations attempted by the last SSSP launch */
    int64_t long_paths;       /* pairs with more hops than the in-register path buffer */
    int64_t errors;           /* pairs with a missing edge (no self loop etc.) */
    double phase_ms[4];       /* SSSP kernel time summed over workgroups: init, near-far SSSP,
                                 parent derivation, per-target epilogue */
    int64_t near_iterations;  /* near-phase iterations summed over sources */
    int64_t far_splits;       /* buckets taken from the bucket window, summed over sources */
    int64_t slots;            /* concurrent SSSP workgroups of the last launch */
    int64_t events[8];        /* queue entries expanded, tail relaxations, tail improvements,
                                 window entries taken, overflow entries refilled, parent-pass
                                 vertices, relaxations onto settled tail vertices, stale
                                 entries skipped (events 1, 2, 6, 7 need option "events") */
    int64_t far_scan_sources; /* sources that overflowed a queue (scanning buckets instead) */
    double split_ms;          /* bucket changes + refills, summed over workgroups (in phase 1) */
    int64_t batch;            /* sources per SSSP workgroup of the last build (0: complete graph) */
    int64_t lds_hubs;         /* LDS-resident hub rows of the last SSSP launch */
    int64_t replay_rows;      /* rows recomputed by the exact igraph heap replay (rows with a
                                 d-tied parent on a target chain; every row of a directed graph) */
    double replay_ms;         /* event-timed duration of the heap-replay launch */
    int64_t replay_pops;      /* heap operations of the replay, summed over its rows: pops, */
    int64_t replay_pushes;    /*   pushes (first reach) and */
    int64_t replay_modifies;  /*   modifies (strict improvement of a queued vertex) */
    int64_t replay_slots;     /* concurrent replay wavefronts of the last launch */
    int64_t route_bad_packets; /* packets with a column outside [0, A), not routed (delivered 0,
                                  time 0, state unchanged), since the last table build */
    int64_t devices;          /* GPUs that built the last table (option "devices") */
    double exchange_ms;       /* RCCL all-gather + all-reduce(min) of that build (wall) */
    double parent_phase_ms[4]; /* batch kernel parent pass, summed over workgroups: walks, merged
                                  row scans, recount + finalize, next level */
    int64_t replay_lines[6];  /* profiling builds (-DSHD_RP_LINES=1) only, else 0: 64-B lines the
                                 replay touched in HBM -- sink loads, sink stores, shift-up loads,
                                 shift-up stores, relaxation loads, relaxation stores */
    int64_t batch_fill;       /* sources per batch of the last batched build (<= batch) */
    double replay_phase_ms[4]; /* profiling builds (-DSHD_RP_TIME=1) only, else 0: replay wall
                                  time summed over wavefronts -- sink, row + record loads, heap
                                  operations of the relaxation, init + epilogue */
    int64_t replay_sink_rounds; /* same builds: sink round trips and heap size, summed over pops, */
    int64_t replay_heap_sum;
    double replay_sink_ms[3];   /*   the sink's LDS walk, HBM rounds and moves, */
    int64_t replay_pf_hits;     /*   pops whose row bounds were prefetched */
    int64_t replay_skips;       /* replay relaxations into vertices the landmark bound proves
                                   popped (their vertex record is not read) */
    int64_t tie_dense;          /* 1: the last build ran every row through the replay because the
                                   topology is tie-dense (option "tie_dense") */
    double batch_wave_ms[6];    /* profiling builds (-DSHD_BATCH_TIME=1) only, else 0: batch
                                   kernel wave time summed over waves -- tail iterations' chunk
                                   loads, phase A, phase B, then the same for hub iterations */
    int64_t batch_rounds;       /*   phase-B rounds and the (edge, source) pairs that reached phase B */
    int64_t batch_edges_b;
    int64_t target_kappa_iters; /* iterations of the target-aware kappa fixpoint of the last target
                                   set (option "target_kappa") */
    double target_prep_ms;      /* wall time of that target-set preparation (target bits + kappa
                                   fixpoint in the relaxation copy; once per target set) */
    /* cold-build breakdown (the once-per-topology work a Shadow run pays before its first table,
       shd-topology.c:757-794 times the reference's equivalent inside the run): */
    double csr_ms;              /* wall time of the graph preparation (upload, relabel, CSR, h0
                                   distances, kappa-sorted copy); 0 when it ran in an earlier build */
    double csr_host_ms;         /*   of which CPU work on the host (not waiting for the GPU) */
    double csr_copy_ms;         /*   of which host <-> device copies (the parsed edge arrays in,
                                     perm / inv / pi / h0-tree parents out) */
    int64_t csr_h0_rounds;      /*   frontier rounds of its h0 distances (pi = d(h0, .)) */
    double order_ms;            /* host: source order, batch order and bucket shifts of the last
                                   batched build */
    double replay_prep_ms;      /* wall time of the heap replay's incidence CSR (once per topology) */
    int64_t touched_lines;      /* tail distance lines the batches of the last build reset (only the
                                   lines a batch lowered from +inf are reset for the next one) */
    int64_t csr_host_runs;      /* host-side graph preparations in the last build (a multi-GPU
                                   build prepares once and shares it with its peer engines) */
    double workspace_ms;        /* wall time of allocating + initialising the SSSP workspace
                                   (first build, or a layout change) */
    double csr_step_ms[8];      /* graph preparation steps (wall): upload of the parsed edges,
                                   degrees + relabel, adjacency rows, h0 distances, h0 tree +
                                   record fields, kappa-sorted copy, host copies out, (unused) */
    double module_load_ms;      /* device init: loading the kernels' code objects and the first
                                   segmented sort's host setup (once per engine, before its
                                   first build) */
    double build_wall_ms;       /* wall time of the last whole-table build (topology_getLatency's
                                   lazy build, shdtopo_build / shdtopo_rebuild) */
    int64_t walk_steps;         /* parent-pass walk steps (pairs resolved) of the last build */
    double build_step_ms[8];    /* wall checkpoints of the last whole-table build: device init,
                                   geometry + table buffers, preparation up to the SSSP launch
                                   (graph, workspace, target set, order), the SSSP kernel, the tie
                                   replay + rest of the rows, statistics, (unused) x 2 */
    int64_t exchange_kind;      /* the last build's row exchange (option "exchange"): 0 none (one
                                   device), 1 RCCL all-gather + all-reduce(MIN) after every shard,
                                   2 push: each shard copied into the other devices' tables (peer
                                   DMA) as soon as it is done (engines sharing a device, RCCL
                                   unavailable, or exchange = 2) */
    int64_t walk_kinds[4];      /* of the walk steps: parents certified by the h0-tree guess, by a
                                   tail's recorded improver, by a hub's recorded improver, and pairs
                                   sent to the merged row scans */
    double build_wait_ms;       /* the last whole-table build's wait for the build lock (the
                                   attach-time preparation thread, or another builder) */
    double attach_prep_ms;      /* wall time of the attach-time preparation (option
                                   "prepare_on_attach": device init + graph preparation in a
                                   background thread from the first attach on, overlapping the
                                   host's attach phase; 0 if it did not run) */
    int64_t replay_int_keys;    /* 1: the last replay ran on u32 heap keys (every latency an
                                   integer, V x max latency < 2^32 - 1: exact), 0: f64 keys */
    int64_t tie_probe_rows;     /* the last build's tie probe (integer latencies, before the first
                                   batched build): sample rows run through the batch kernel, */
    int64_t tie_probe_flagged;  /*   of which crossing a d-tied parent (>= 90 %: tie-dense, every
                                     row goes straight to the heap replay) */
    double tie_probe_ms;        /*   and its wall time */
    double first_attach_to_table_ms; /* wall time from the first attach to the first table
                                        installed (once per topology; 0 before) */
    int64_t exchange_bytes;     /* bytes each device received in the last row exchange (all-gather
                                   of the other devices' rows, hops and row minima) */
    int64_t csr_host_runs_total; /* host-side graph preparations since the topology was loaded,
                                    the owner's and every peer engine's, the attach-time
                                    preparation thread's included */
    int64_t sweep_events[4];    /* profiling builds (-DSHD_BATCH_TIME=1) only, else 0: the batch
                                   kernel's phase-B rounds holding a tail-target pair, tail-target
                                   pairs, hub-target pairs, (unused) */
    int64_t write_lines[16];    /* profiling builds (-DSHD_BATCH_WRCOUNT=1) only, else 0: 64-B lines
                                   the batch kernel's stores and atomics touched, by category
                                   (topo_sssp_batch.hip WL_*): relaxation atomicMin, tie tags,
                                   improver hints, pending atomics, touched atomics, near-mask
                                   atomics; mask stores; pending words; line reset; touched-word
                                   clears; pair records; parent scratch; table output; hub rows and
                                   hints; queue appends; other */
    int64_t read_lines[8];      /* the same builds: 64-B lines read, by category (RL_*): phase-B
                                   pre-checks, phase-A records, chunk loads, sweeps, parent walks,
                                   epilogue, reset, other (hint pass, row scans) */
    double attach_prep_step_ms[4]; /* the attach-time preparation's parts (wall): device init (HIP
                                      queues, code objects), graph preparation, edge scan, the
                                      batched SSSP's workspace (allocation + initialisation) */
    int64_t pair_matrix_builds; /* complete topologies: times the resident A x A direct-edge
                                   matrices were (re)built (once per attached set; cumulative) */
    double device_kernel_ms[8]; /* the last multi-device build (option "devices"), per device slot
                                   (first 8): event time of its row shard's kernels (SSSP or pair
                                   kernel, + heap replay), */
    double device_build_ms[8];  /*   wall time of its row shard's build, */
    int64_t device_rows[8];     /*   and its rows */
    int64_t dev_inits;          /* device initialisations of this topology (HIP stream, events, code
                                   objects): 1, or 2 when the "device" option moved it */
    double init_bg_ms;          /* wall time of topology_new's background device init (overlaps the
                                   GraphML parse; 0 if it did not run) */
    double path_seconds_total;  /* shortestPathTotalTime of the reference (shd-topology.c:792): wall
                                   seconds of every table / row build so far */
    int64_t paths_computed;     /* shortestPathCount (shd-topology.c:793): source rows built so far;
                                   both are logged at topology_free (:445-446) */
    int64_t batch_layout_measured; /* 1: the last batched launch used the measured layout (option
                                      "balance": batches sized / ordered by the sources' costs
                                      from earlier builds' batch times), 0: the grouping order */
    int64_t batches;            /*   batches of that launch */
    int64_t rows_to_host;       /* getters (topology_getLatency & co.): table rows copied to the
                                   host on their first read, cumulative (16 A bytes each; the
                                   getters never copy the whole A x A table) */
    double rows_to_host_ms;     /*   and the wall time of those copies */
    int64_t prep_trigger;       /* what started the background graph preparation (attach_prep_ms):
                                   0 none, 1 the first attach, 2 topology_new (right after the
                                   parse; SHDTOPO_NO_LOAD_PREP=1 turns that off) */
    double exchange_exposed_ms; /* the last multi-device build: wall time from the last shard's
                                   rows to the end of the exchange (the part of exchange_ms no
                                   kernel hid; exchange_kind 2 overlaps the slower shards) */
    int64_t workspace_bytes;    /* HBM held by the batched SSSP's workspace (all slots) */
    int64_t peeled_targets;     /* the last batched build: targets with one non-loop edge, resolved
                                   from their uplink instead of the graph search (option
                                   "leaf_targets"; 0 when off or the topology is directed) */
} ShdStats;
int shdtopo_get_stats(Topology* top, ShdStats* out);

/* Test hook: the measured batch layout (option "balance") for per-position
 * costs cost[rows] (grouping order) with a batch's fixed part `fixed`, batch fill `fill`, `slots`
 * workgroups and batch width `batch`.  order u32[rows] receives the grouping positions in launch
 * order, starts u32[rows + 1] the batch starts (*nbatches + 1 entries): one round of the slots =
 * runs of the grouping order minimising the largest predicted batch; several rounds = batches of
 * `fill` consecutive positions, longest predicted first, the ragged one last.  Returns 0, or -1
 * when no layout applies (the build then keeps the grouping order).  Host-only: no device use. */
int shdtopo_test_batch_layout(const double* cost, int64_t rows, double fixed, int fill, int slots,
                              int batch, uint32_t* order, uint32_t* starts, int64_t* nbatches);

/* Test hook: the seed of the batch kernel's landmark bound (option "h0_seed") for a source whose
 * prepared distance to the landmark is p on a graph of `vertices` vertices: 0 for p = 0, +inf for
 * a p that is not finite, else p (1 + max(1e-9, 4 vertices 2^-53)) rounded up.  Host-only. */
double shdtopo_test_h0_seed(double p, int64_t vertices);

/* Test hook: the segmented sort of the target-aware re-sort on HIP device 0 -- nseg rows
 * (rowptr u32[nseg + 1] over n f32 keys) each sorted ascending and stably; keys_out receives the
 * sorted keys, idx_out their input positions.  reference = 1 runs the whole-adjacency hipcub
 * segmented radix sort the library's kernels replace (the order they must reproduce).  Returns 0,
 * -1 on bad arguments, or a HIP error. */
int shdtopo_test_segsort(const uint32_t* rowptr, int64_t nseg, const float* keys, int64_t n,
                         int reference, float* keys_out, uint32_t* idx_out);

/* Test hook: run the exact heap replay (igraph_get_shortest_paths_dijkstra restated on the GPU)
 * from vertex `src` over the current attached set.  full = 1 runs to an empty heap instead of
 * stopping when every attached vertex is popped.  dist f64[V] (-1 = unreached) and parent int32[V]
 * (-1 = none) receive the replay's result in original vertex ids.  Returns 0 or an error. */
int shdtopo_replay_source(Topology* top, int32_t src, int full, double* dist, int32_t* parent);

/* ---- route tracing: the vertex / edge path behind a table entry ----
 * The reference logs it at debug level for every pair it computes (shd-topology.c:594,644,
 * 654-656).  A trace answers "which route does host A take to host B, and which link contributes
 * the 40 ms" without touching the table. */
typedef struct {
    int64_t offset;      /* first entry of this route in vertices[] / edges[]; -1 if not written */
    int32_t hops;        /* edges on the route (self pair: 1, the self loop); -1 if not traced    */
    int32_t status;      /* 0 ok, 1 src or dst not attached, 2 unroutable / broken chain,
                            3 route longer than the space left (cap)                             */
    double  latency;     /* re-accumulated along the route, the helper's order and zero rule     */
    double  reliability; /* ((1*(1-p_src))*(1-p_dst))*prod(1-p_e) from the source end            */
} ShdRoute;

/* Trace the routes of n (source, destination) host pairs (IPs in network order; duplicate and
 * unsorted requests are fine).  Route i takes hops + 1 entries at routes[i].offset:
 * vertices[offset .. offset + hops] are original vertex indices, source first, destination last;
 * edges[offset + k] is the edge between vertices[offset + k] and vertices[offset + k + 1] (edge id
 * = document order = igraph's id; of a parallel group the lowest id, as igraph_get_eid), and
 * edges[offset + hops] = -1.  Two hosts on one vertex (or src == dst) take the self loop:
 * vertices [v, v], hops 1; no self loop: status 2.  Offsets are the running sum of hops + 1 over
 * the requests in request order, and the return value is the number of entries all routes need,
 * so a call with cap = 0 (vertices / edges may then be NULL) sizes the buffers.  With a cap that
 * is too small the routes that fit entirely are written; the rest get status 3 and offset -1
 * (hops, latency and reliability still filled), and nothing at or beyond cap is touched.
 * Requests with status 1 or 2 have hops -1, offset -1, latency = reliability = -1.0.
 *
 * The route is always the forward route of the SOURCE's row for the current attached set:
 * latency, reliability and hops equal shdtopo_table_to_host at [col(src)][col(dst)] bit for bit.
 * In lazy mode on an undirected topology topology_getLatency(a, b) may be answered from row b
 * (first-rooted-wins, shd-topology.c:896-915) and then equals trace(b, a), not trace(a, b).
 *
 * SSSP topologies: the distinct sources are taken in chunks (option "trace_chunk"; at most the
 * replay's wavefront slots and the batch kernel's slots x sources per batch).  A chunk runs the
 * batch kernel once on its sources (option "trace_batch" = 1, the default; milliseconds per
 * source) and walks the parent records that launch leaves; a source whose row crosses a tied
 * parent -- the rows a table build hands to the heap replay -- or has a broken requested chain
 * runs through the exact heap replay instead (seconds per source at a million vertices,
 * DESIGN.md 3.6), and so does every source when the batch kernel does not apply: a tie-dense
 * topology, a multigraph, "replay_all", a target set the relaxation copy was not prepared for
 * (hosts attached since the last build), or "trace_batch" = 0.  Both paths give the same bytes.
 * The first trace uploads the edge ids (4 B per adjacency entry).  Complete
 * topologies (_topology_lookupPath, :835-873: one hop over the direct edge) are answered on the
 * host from the parsed graph: no device, no table.  A multi-device topology traces on its first
 * device.  A trace materialises no lazy row, pushes no minimum, neither invalidates nor rebuilds
 * the table and leaves ShdStats as it was.  Returns a negative value on an error (-1: bad
 * arguments). */
int64_t shdtopo_trace_routes(Topology* top, const uint32_t* srcIP, const uint32_t* dstIP, int64_t n,
                             ShdRoute* routes, int32_t* vertices, int32_t* edges, int64_t cap);
/* Host-only: the text of the reference's debug line for route r (status 0, written) --
 * "shortest path %s-->%s (%i-->%i) is %f ms with %f loss, path: %s" with the vertices' GraphML
 * ids and, per hop, "--[%f,%f]-->%s" = [edge latency, 1 - edge packetloss].  Writes at most cap
 * bytes (NUL-terminated when cap > 0) and returns the length needed (without the NUL), or -1. */
int64_t shdtopo_format_route(Topology* top, const ShdRoute* r, const int32_t* vertices,
                             const int32_t* edges, char* buf, size_t cap);
/* the last trace's own counters (ShdStats is not touched by a trace) */
typedef struct {
    double total_ms;        /* wall time of the call */
    double replay_ms;       /* event time of its heap-replay launches only */
    double trace_kernel_ms; /* event time of route_trace_kernel, its scans, placement and scatter */
    double ids_ms;          /* wall time of the edge-id upload (first trace of a topology, else 0) */
    int64_t requests;       /* n */
    int64_t sources;        /* distinct source vertices of the call, either path */
    int64_t chunks;         /* source chunks */
    int64_t entries;        /* the call's return value */
    double batch_ms;        /* event time of the batch kernel's keep launches */
    int64_t batch_sources;  /* distinct sources answered from the batch kernel's parent records */
    int64_t batch_fallback; /* sources that ran a keep launch and then went to the heap replay */
} ShdTraceStats;
int shdtopo_trace_stats(Topology* top, ShdTraceStats* out);

/* ---- link load: per-edge and per-vertex traffic of a set of flows ----
 * "Which links carry my traffic": for n flows (source host, destination host, weight; IPs in
 * network order, duplicates and any order are fine) the weight that crosses every edge and arrives
 * at every vertex.  Route i is exactly the route shdtopo_trace_routes reports for
 * (srcIP[i], dstIP[i]): the forward route of the source's row for the current attached set, each
 * hop over the igraph_get_eid edge (the lowest id of a parallel group), the self loop for two
 * hosts on one vertex or src == dst.
 *
 * For every hop from vertex a to vertex b over edge e (ids in document order):
 *   edgeLoad[e] += w       when a == eu[e]: the forward half -- also every self loop and every
 *                          arc of a directed topology;
 *   edgeLoad[E + e] += w   otherwise: the reverse half (all zero on a directed topology);
 *   vertexLoad[b] += w     the weight arriving at b (original vertex ids): every vertex of the
 *                          route but its first; a self pair arrives once, over its loop.
 * weight = NULL counts 1 per flow (packets); weight = payloadLength gives bytes.  Sums are
 * unsigned 64-bit and wrap, so they do not depend on request order, chunking or scheduling.
 * edgeLoad (u64[2 E]) and vertexLoad (u64[V]) are overwritten, not accumulated into; either may
 * be NULL.  Requests with an unattached end, and unroutable ones (a broken chain, a self pair
 * without a self loop), are counted in the statistics and skipped.  Returns the number of flows
 * that contributed, or a negative error (-1: bad arguments -- NULL top, n < 0, a NULL IP array
 * with n > 0).
 *
 * SSSP topologies: the distinct sources are taken in chunks (option "trace_chunk") and get their
 * chains as in a trace: from the batch kernel's parent records where that is exact (option
 * "trace_batch"), else from the exact heap replay.  The accumulation itself is microseconds to
 * milliseconds (option "load_walk" selects between the per-request walk and the
 * tree sums; the tree sums keep their state in the replay's records, so "load_walk" = 0 replays
 * every source).  Complete topologies are
 * answered on the host from the parsed graph: no device is used.  A multi-device topology runs on
 * its first device.  Like a trace, the call materialises no lazy row, pushes no minimum, neither
 * invalidates nor rebuilds the table and leaves ShdStats as it was. */
typedef struct {
    double  total_ms;        /* wall time of the call */
    double  replay_ms;       /* event time of its heap-replay launches only */
    double  load_kernel_ms;  /* event time of the accumulation kernels (everything but the replay) */
    double  ids_ms;          /* edge-id upload, first trace/load of a topology, else 0 */
    int64_t requests;        /* n */
    int64_t routed;          /* requests that contributed */
    int64_t unattached;      /* requests with an unattached end (contribute nothing) */
    int64_t broken;          /* unroutable / broken chain / self pair without a self loop */
    int64_t sources;         /* distinct source vertices of the call, either path */
    int64_t chunks;          /* source chunks */
    int64_t tree_vertices;   /* sum over sources of the vertices in the union of its requested chains
                                (the source aside: = adds into the edge accumulators, self pairs
                                apart); 0 for the per-request walk */
    uint64_t hop_weight;     /* sum over routed requests of weight x hops (= sum of edgeLoad) */
    double  batch_ms;        /* event time of the batch kernel's keep launches */
    int64_t batch_sources;   /* distinct sources answered from the batch kernel's parent records */
    int64_t batch_fallback;  /* sources that ran a keep launch and then went to the heap replay */
} ShdLoadStats;

int64_t shdtopo_link_load(Topology* top, const uint32_t* srcIP, const uint32_t* dstIP,
                          const uint64_t* weight /* NULL: 1 each */, int64_t n,
                          uint64_t* edgeLoad /* u64[2 * E], may be NULL */,
                          uint64_t* vertexLoad /* u64[V], may be NULL */);
int shdtopo_link_load_stats(Topology* top, ShdLoadStats* out);

/* ---- link crossings: which flows cross a set of watched links and routers ----
 * Link load's inverse question -- "which of my flows go over this link or through this router":
 * the blast radius of a link before it is failed, the circuits that share a bottleneck.  For n
 * flows (source host, destination host, weight; IPs in network order, duplicates and any order are
 * fine), ne watched edges (edge ids, document order) and nv watched vertices (original vertex ids)
 * the call reports every hop of a flow's route that goes over a watched edge or arrives at a
 * watched vertex, without writing a single route out.
 *
 * Flow i's route is exactly the route shdtopo_trace_routes reports for (srcIP[i], dstIP[i]): the
 * forward route of the source's row for the current attached set, each hop over the igraph_get_eid
 * edge (the lowest id of a parallel group -- watching a higher id of the group reports nothing),
 * the self loop (hop 0) for two hosts on one vertex or src == dst.  For the hop number `hop` from
 * vertex a = vertices[hop] to b = vertices[hop + 1] over edge e:
 *   e == watchEdge[k]    one record {i, k, hop, reverse}: either direction counts, reverse = 1 when
 *                        a != eu[e] (link load's reverse half; 0 for every self loop and every arc
 *                        of a directed topology);
 *   b == watchVertex[k]  one record {i, ne + k, hop, 0}: link load's vertexLoad rule -- every
 *                        vertex of the route but its first; a self pair arrives once, over its loop.
 * A hop with both yields two records, the edge record first.  Records are ordered by flow
 * ascending, then hop ascending, then edge before vertex; flowOffset[i] (i64[n + 1], may be NULL)
 * is the running sum of the flows' record counts and flowOffset[n] the return value, the total
 * number of crossings.  The bytes of out do not depend on chunking, scheduling, "trace_batch" or
 * which chain source served a flow.  A call with cap = 0 (out may then be NULL) sizes the buffer.
 * With a cap that is too small flow i's records are written iff flowOffset[i + 1] <= cap and
 * nothing at or beyond cap is touched; flowOffset, watchCount, watchWeight and the return value
 * are complete regardless.
 *
 * watchCount[k] (u64[ne + nv], may be NULL) is the number of records of watch k, watchWeight[k]
 * (the same) the sum of their flows' weights (weight = NULL: 1 each), unsigned 64-bit and
 * wrapping: for an edge watch edgeLoad[e] + edgeLoad[E + e] of shdtopo_link_load on the same
 * flows, for a vertex watch vertexLoad[v].  Requests with an unattached end, and unroutable ones
 * (a broken chain, a self pair without a self loop), contribute nothing and are counted in the
 * statistics.  ne + nv == 0 is valid: the call returns 0 and every offset is 0 (on an SSSP topology
 * nothing is walked then: routed and broken stay 0).
 *
 * Returns a negative value on an error; -1: bad arguments -- NULL top; n, ne, nv or cap negative;
 * a NULL IP array with n > 0; a NULL watch array with a positive count; cap > 0 with NULL out; an
 * edge id outside [0, E) or a vertex id outside [0, V); a duplicate id within one watch list.
 *
 * SSSP topologies: the distinct sources are taken in chunks (option "trace_chunk") and get their
 * chains as in a trace: from the batch kernel's parent records where that is exact (option
 * "trace_batch"), else from the exact heap replay; option "load_walk" has no meaning here.  The
 * walks themselves are microseconds to milliseconds.  Complete topologies are
 * answered on the host from the parsed graph (one hop over the direct edge): no device is used.
 * A multi-device topology runs on its first device.  Like a trace and a load, the call holds the
 * build lock, materialises no lazy row, pushes no minimum, neither invalidates nor rebuilds the
 * table and leaves ShdStats, the trace statistics and the load statistics as they were. */
typedef struct {
    int32_t flow;     /* request index i */
    int32_t watch;    /* k in [0, ne): watchEdge[k];  ne + k: watchVertex[k] */
    int32_t hop;      /* 0-based hop from the source: the hop vertices[hop] -> vertices[hop + 1]
                         of the route shdtopo_trace_routes reports for the flow */
    int32_t reverse;  /* edge watch: 1 when the hop does not leave eu[e] (link load's reverse
                         half); 0 for self loops, directed arcs and every vertex watch */
} ShdCrossing;
typedef struct {
    double  total_ms;        /* wall time of the call */
    double  replay_ms;       /* event time of its heap-replay launches only */
    double  kernel_ms;       /* event time of everything but the replay and the keep launches */
    double  ids_ms;          /* edge-id upload, first trace/load/crossings of a topology, else 0 */
    int64_t requests;        /* n */
    int64_t routed;          /* requests whose route was walked */
    int64_t unattached;      /* requests with an unattached end (contribute nothing) */
    int64_t broken;          /* unroutable / broken chain / self pair without a self loop */
    int64_t sources;         /* distinct source vertices of the call, either path */
    int64_t chunks;          /* source chunks */
    int64_t crossings;       /* the call's return value */
    int64_t flows_hit;       /* flows with at least one record */
    double  batch_ms;        /* event time of the batch kernel's keep launches */
    int64_t batch_sources;   /* distinct sources answered from the batch kernel's parent records */
    int64_t batch_fallback;  /* sources that ran a keep launch and then went to the heap replay */
} ShdCrossStats;

int64_t shdtopo_link_crossings(Topology* top, const uint32_t* srcIP, const uint32_t* dstIP,
                               const uint64_t* weight /* NULL: 1 each */, int64_t n,
                               const int32_t* watchEdge, int64_t ne /* edge ids, document order */,
                               const int32_t* watchVertex, int64_t nv /* original vertex ids */,
                               int64_t* flowOffset /* i64[n + 1], may be NULL */,
                               ShdCrossing* out, int64_t cap,
                               uint64_t* watchCount, uint64_t* watchWeight
                               /* u64[ne + nv] each, may be NULL */);
int shdtopo_link_crossings_stats(Topology* top, ShdCrossStats* out);

/* ---- link timeline: per-time-bin traffic on watched links and routers ----
 * The trace, the load and the crossings ignore time.  The packets of a scheduler window carry an
 * emission time (TopoPacketIn.now), and this call says when, inside the window, their bytes hit a
 * watched link or router: for n flows (source host, destination host, weight, emission time now
 * in ns), ne watched edges and nv watched vertices (as shdtopo_link_crossings) it sums the flows'
 * weights per watch and time bin, without writing a single route out.
 *
 * Flow i's route is exactly the route shdtopo_trace_routes reports for (srcIP[i], dstIP[i]): the
 * forward route of the source's row for the current attached set, each hop over the igraph_get_eid
 * edge (the lowest id of a parallel group -- watching a higher id of the group reports nothing),
 * the self loop for two hosts on one vertex or src == dst.  For hop k from vertex a to b over edge
 * e let pre_k be the latency of hops 0 .. k - 1 and post_k that of hops 0 .. k, both accumulated
 * from 0.0 by one IEEE add per hop in route order (the trace's accumulation; the 0 -> 1 override
 * of a whole route's latency is not applied to prefixes).  With ns(x) = (uint64_t)ceil(x *
 * 1000000.0), the conversion of topology_routePacketBatch, and u64 arithmetic,
 *   enter_k = now[i] + ns(pre_k)      arrive_k = now[i] + ns(post_k)
 *   e == watchEdge[j]    weight[i] goes to row j when the hop leaves eu[e] (every self loop and
 *                        every arc of a directed topology), else to row ne + j (all zero on a
 *                        directed topology), timed enter_k;
 *   b == watchVertex[j]  weight[i] goes to row 2 ne + j, timed arrive_k: link load's vertexLoad
 *                        rule -- every vertex of the route but its first; a self pair arrives
 *                        once, over its loop.
 * A hit with time t lands in outside[row][0] when t < t0, else in outside[row][1] when
 * (t - t0) / binNs >= nbins, else in bins[row][(t - t0) / binNs].  bins is u64[(2 ne + nv) x
 * nbins], row-major, outside u64[(2 ne + nv) x 2]; both are overwritten, not accumulated into.
 * Sums are unsigned 64-bit and wrap, so the result does not depend on chunking, scheduling,
 * "trace_batch" or which chain source served a flow.  now = NULL is 0 each: the bins are then
 * "time since emission".  Summed over its bins and its outside pair a row holds watchWeight of
 * shdtopo_link_crossings on the same flows and watches (fwd + rev for an edge watch).
 *
 * Returns the number of hits, in range or not: the total of shdtopo_link_crossings for the same
 * flows and watches.  Requests with an unattached end, and unroutable ones, contribute nothing and
 * are counted in the statistics.  ne + nv == 0 is valid: the call returns 0 and walks nothing.
 * Negative on an error; -1: bad arguments -- NULL top; n, ne, nv or nbins negative; binNs == 0
 * with nbins > 0; a NULL IP array with n > 0; a NULL watch array with a positive count; NULL bins
 * with (2 ne + nv) x nbins > 0; an edge id outside [0, E) or a vertex id outside [0, V); a
 * duplicate id within one watch list.
 *
 * Not modelled: the sender's Bernoulli drop (filter by `delivered` of the packet batch if wanted),
 * the inter-host clamp and any queueing.  Shadow delivers a packet in one event at the
 * destination; the intermediate times are this model's interpolation of that event along the
 * route, not times Shadow itself would ever observe.
 *
 * SSSP topologies: chunks and chain sources as shdtopo_link_crossings; option "load_walk" has no
 * meaning here.  A flow without a hit costs one walk; a flow with one parks its hops (8 B each) in
 * device memory and is walked again source -> destination.  Complete topologies
 * are answered on the host from the parsed graph (one hop over the direct edge: enter = now,
 * arrive = now + ns(0.0 + latency)): no device is used.  A multi-device topology runs on its first
 * device.  Like a trace, a load and the crossings, the call holds the build lock, materialises no
 * lazy row, pushes no minimum, neither invalidates nor rebuilds the table and leaves ShdStats and
 * the trace, load and crossings statistics as they were. */
typedef struct {
    double  total_ms;        /* wall time of the call */
    double  replay_ms;       /* event time of its heap-replay launches only */
    double  kernel_ms;       /* event time of everything but the replay and the keep launches */
    double  ids_ms;          /* edge-id upload, first trace/load/crossings/timeline, else 0 */
    double  batch_ms;        /* event time of the batch kernel's keep launches */
    int64_t requests;        /* n */
    int64_t routed;          /* requests whose route was walked */
    int64_t unattached;      /* requests with an unattached end (contribute nothing) */
    int64_t broken;          /* unroutable / broken chain / self pair without a self loop */
    int64_t sources;         /* distinct source vertices of the call, either path */
    int64_t chunks;          /* source chunks */
    int64_t batch_sources;   /* distinct sources answered from the batch kernel's parent records */
    int64_t batch_fallback;  /* sources that ran a keep launch and then went to the heap replay */
    int64_t hits;            /* the call's return value */
    int64_t flows_hit;       /* flows with at least one hit */
    int64_t in_range;        /* hits (not weights) that landed in a bin */
    int64_t before;          /* hits before t0 */
    int64_t after;           /* hits at or after the last bin */
    int64_t staged_hops;     /* hops parked in device memory (flows with a hit, self pairs aside) */
} ShdTimelineStats;

int64_t shdtopo_link_timeline(Topology* top, const uint32_t* srcIP, const uint32_t* dstIP,
                              const uint64_t* weight /* NULL: 1 each */,
                              const uint64_t* now /* ns; NULL: 0 each = "time since emission" */,
                              int64_t n,
                              const int32_t* watchEdge, int64_t ne /* edge ids, document order */,
                              const int32_t* watchVertex, int64_t nv /* original vertex ids */,
                              uint64_t t0, uint64_t binNs, int64_t nbins,
                              uint64_t* bins /* u64[(2 ne + nv) * nbins], row-major; may be NULL
                                                iff that is 0 */,
                              uint64_t* outside /* u64[(2 ne + nv) * 2]: {before t0, at or after
                                                   the last bin}; may be NULL */);
int shdtopo_link_timeline_stats(Topology* top, ShdTimelineStats* out);

/* ---- link monitor: running per-bin link traffic fed by packet windows ----
 * shdtopo_link_timeline answers one call: it walks every flow's route and overwrites its outputs.
 * A link monitor is the same question kept open across a run.  It is a persistent object of its
 * topology that holds a watch set (edges and vertices, as shdtopo_link_crossings), a bin geometry
 * (t0, binNs, nbins, as shdtopo_link_timeline), cumulative bins in device memory and a
 * device-resident hit index over the table's A x A column pairs.
 *
 * After any sequence of feeds the monitor's bins and outside pairs equal, byte for byte, what
 * shdtopo_link_timeline returns for the concatenation of all fed packets that were not filtered
 * out, with the same watches and bins: rows, hop rules, ns(), the accumulation order of the prefix
 * latency, self pairs (two hosts on one vertex share a column: a self pair) and the wrapping u64
 * arithmetic are those of the "link timeline" section above.  Nothing new is modelled.
 *
 * For a fixed watch set and attached set, enter_k - now and arrive_k - now of a hit depend on the
 * (source column, destination column) pair alone.  shdtopo_monitor_prepare walks the routes once
 * with the timeline's machinery (sources in blocks of one chunk; options "trace_chunk" and
 * "trace_batch" keep their meaning) and keeps, per pair, its hits {row, offset ns} in hop order,
 * within a hop the edge record before the vertex record: 16 B a record and one i64 offset per
 * pair.  A feed then costs one gather and one u64 atomic add per hit per packet.
 * Complete topologies build the index on the host from the parsed graph (one hop over the direct
 * edge: offset 0, arrival ns(0.0 + latency); a self pair over its loop); their host feeds use no
 * device, shdtopo_monitor_feed_device uploads that index once and runs the same kernel.
 *
 * Monitors are small integer ids of their topology, not pointers: a stale id (freed) or the id of
 * another topology's monitor returns -1 from every call and dereferences nothing.
 * shdtopo_topology_free releases every remaining monitor.
 *
 *   shdtopo_monitor_new      id >= 0; -1 on the argument errors shdtopo_link_timeline lists (n and
 *                            the IP and output arrays aside).  ne + nv == 0 is valid: such a
 *                            monitor builds no index and every feed returns 0.  Uses no device.
 *   shdtopo_monitor_prepare  builds or rebuilds the index for the current column geometry (the
 *                            columns shdtopo_route_batch_device sees, those deferred by
 *                            shdtopo_window_hold included); returns the number of records.  The
 *                            feeds call it themselves when the index is missing or stale (the
 *                            attached set or the geometry moved since it was built).  The bins
 *                            survive a rebuild: rows are per watch, not per column.  -5: the
 *                            index does not fit option "monitor_index_mb" (a double, MB; 0, the
 *                            default: half of the device memory free at prepare) -- found by the
 *                            count pass, before the records of the block that exceeds it are
 *                            allocated; the monitor stays unprepared, later feeds return -5 and
 *                            the bins are untouched.
 *   shdtopo_monitor_feed     host arrays; the IPs resolve exactly as in shdtopo_link_timeline (a
 *                            request with an unattached end contributes nothing and is counted).
 *                            Packets with delivered[i] == 0 are skipped.  Returns this feed's
 *                            hits, in range or not.  -1: NULL IP array with n > 0, n negative.
 *   shdtopo_monitor_feed_vertices  the same with original vertex ids (-1 = not attached).
 *   shdtopo_monitor_feed_device    the arrays of shdtopo_route_batch_device, resident in device
 *                            memory; enqueued on `stream` (NULL: the library's), not awaited;
 *                            returns 0 or a negative error.  A column outside [0, A) is skipped
 *                            and counted (bad_columns), nothing is read through it.  The monitor
 *                            owns one event: each device feed records it on its stream, a feed
 *                            on another stream than the previous one first waits on it.
 *   shdtopo_monitor_read     the cumulative bins, shapes as shdtopo_link_timeline (either may be
 *                            NULL).
 *   shdtopo_monitor_reset    zeroes the bins and the cumulative counters; keeps the index.
 *   shdtopo_monitor_stats    counters and index facts, below.
 *   shdtopo_monitor_export_index  test hook: pair (s, d) owns records [pairOff[s A + d],
 *                            pairOff[s A + d + 1]); returns the number of records (prepares if
 *                            needed); arrays are written when cap >= that (cap = 0 sizes them;
 *                            any pointer may be NULL).
 * read, stats, reset, prepare, export_index and free synchronise the monitor's event and the
 * library's stream first.  The n == 0 feed and the feeds of a monitor without watches launch
 * nothing.
 *
 * Every call takes the build lock.  Like the rest of the family a monitor materialises no lazy
 * row, pushes no minimum, neither invalidates nor rebuilds the table, and leaves ShdStats and the
 * trace, load, crossings and timeline statistics as they were.  A multi-device topology monitors
 * on its first device. */
typedef struct {
    double  prepare_ms;          /* wall time of the last prepare */
    double  replay_ms;           /* of it: event time of the heap-replay launches */
    double  kernel_ms;           /* of it: event time of everything but replay and keep launches */
    double  batch_ms;            /* of it: event time of the batch kernel's keep launches */
    double  feed_kernel_ms;      /* event time of the last feed's kernel (0: none, host walk) */
    /* cumulative since monitor_new / monitor_reset */
    int64_t hits, flows_hit, in_range, before, after;
    int64_t fed;                 /* packets looked up in the index */
    int64_t skipped_undelivered; /* delivered[i] == 0 */
    int64_t unattached;          /* host feeds: an end that is no column */
    int64_t bad_columns;         /* device feeds: a column outside [0, A) */
    /* the last feed alone */
    int64_t last_hits, last_flows_hit, last_in_range, last_before, last_after;
    int64_t last_fed, last_skipped_undelivered, last_unattached, last_bad_columns;
    int64_t feeds;               /* feed calls since monitor_new */
    /* the index */
    int64_t index_pairs;         /* A x A (0: not prepared) */
    int64_t index_records;
    int64_t index_bytes;         /* offsets + records */
    int64_t prepares;            /* index builds since monitor_new */
    /* the last prepare */
    int64_t sources;             /* source columns walked */
    int64_t chunks;              /* source blocks (one chunk each) */
    int64_t batch_sources;       /* sources answered from the batch kernel's parent records */
    int64_t batch_fallback;      /* sources that ran a keep launch and then the heap replay */
    int64_t broken_pairs;        /* unroutable pairs: no records */
} ShdMonitorStats;

int shdtopo_monitor_new(Topology* top, const int32_t* watchEdge, int64_t ne,
                        const int32_t* watchVertex, int64_t nv, uint64_t t0, uint64_t binNs,
                        int64_t nbins);
int shdtopo_monitor_free(Topology* top, int id);
int64_t shdtopo_monitor_prepare(Topology* top, int id);
int64_t shdtopo_monitor_feed(Topology* top, int id, const uint32_t* srcIP, const uint32_t* dstIP,
                             const uint64_t* weight /* NULL: 1 each */,
                             const uint64_t* now /* ns; NULL: 0 each */,
                             const uint8_t* delivered /* NULL: all */, int64_t n);
int64_t shdtopo_monitor_feed_vertices(Topology* top, int id, const int32_t* srcVertex,
                                      const int32_t* dstVertex, const uint64_t* weight,
                                      const uint64_t* now, const uint8_t* delivered, int64_t n);
int shdtopo_monitor_feed_device(Topology* top, int id, const int32_t* d_srcCol,
                                const int32_t* d_dstCol,
                                const uint32_t* d_payload /* weight; NULL: 1 each */,
                                const uint64_t* d_now /* NULL: 0 each */,
                                const uint8_t* d_delivered /* NULL: all */, int64_t n,
                                void* stream);
int shdtopo_monitor_read(Topology* top, int id, uint64_t* bins, uint64_t* outside);
int shdtopo_monitor_reset(Topology* top, int id);
int shdtopo_monitor_stats(Topology* top, int id, ShdMonitorStats* out);
int64_t shdtopo_monitor_export_index(Topology* top, int id, int64_t* pairOff /* A*A + 1 */,
                                     int32_t* row, uint64_t* offNs, int64_t cap);

/* ---- link failure what-if: derived topologies and a device-side table diff ----
 * The trace, the load, the crossings, the timeline and the monitor describe traffic on the network
 * as it is.  These calls fail links and routers: shdtopo_derive_without makes a second topology
 * without them, carrying the same hosts on the same vertices, and shdtopo_table_diff compares the
 * two routing tables on the device and returns only the pairs that changed.  A full table builds
 * fast enough that recomputing everything after a failure is cheaper than any incremental scheme
 * walking routes, so nothing here is incremental.
 *
 * shdtopo_derive_without returns a new, independent, ordinary Topology (free it with
 * topology_free; the parent may be freed first).  The parent is read under its locks and otherwise
 * left exactly as it was.
 *
 * The derived graph.  A failed edge is removed; a failed vertex loses all its incident edges, its
 * self loop included, and stays behind as an isolated vertex.  Edge ids are the parent's edge ids
 * with the removed ones squeezed out, order kept -- igraph's "lowest edge id" rule and its
 * incidence order are then those of deleting the edges in igraph, ties included.  Vertex ids and
 * all vertex attributes are unchanged.  Nothing is parsed or written: the graph is filtered from
 * the parent's in memory and then goes through the same validation and background preparation as
 * a graph from topology_new.  Every other entry point works on a derived topology unchanged.
 *
 * Validation.  Duplicate ids in the failing lists are allowed.  An empty failing set is valid: a
 * copy whose table is bit-identical to the parent's.  On an error the call returns NULL, *err (may
 * be NULL) receives the code, and no device is initialised:
 *   -1  NULL top; a negative count; a NULL array with a positive count; an edge id outside
 *       [0, E) or a vertex id outside [0, V);
 *   -2  a failed vertex has a host attached in the parent;
 *   -3  the vertices that are not failed do not remain strongly connected (the reference refuses
 *       any other graph; failed vertices are exempt).  A critical log line names the number of
 *       vertices cut off: those outside the largest strongly connected part found.
 * Partitioned networks are out of scope: a failing set that splits the network is refused, not
 * modelled.
 *
 * What is carried over.  Every IP attached in the parent is attached to the same vertex, several
 * hosts on one vertex included, with no random draw: shdtopo_attached_vertices is equal on both
 * and columns mean the same thing.  Columns a window adapter has only deferred are not carried;
 * neither are monitors, windows, lazy rows, statistics or the table.  A failed vertex (of this
 * derivation or of an earlier one) is never an attachment candidate of the derived topology; later
 * topology_attach calls otherwise follow the reference's algorithm and RNG use over the derived
 * graph.  The device ordinal, "abort_on_error" and "lazy" are inherited; every other option
 * starts at its default.
 *
 * shdtopo_edge_origin writes, for each edge id of top, the id of that edge in the root topology
 * (the one that was loaded or synthesised); a derived topology of a derived topology composes the
 * maps, a root topology gives the identity.  Returns E (-1: NULL top) and writes only when
 * cap >= E. */
Topology* shdtopo_derive_without(Topology* top, const int32_t* failEdge, int64_t ne,
                                 const int32_t* failVertex, int64_t nv,
                                 int32_t* err /* may be NULL */);
int64_t shdtopo_edge_origin(Topology* top, int32_t* origin, int64_t cap);

/* shdtopo_table_diff compares the device-resident A x A tables of a and b pair by pair: the
 * {latency, reliability} records and the u16 hops.  Latency and reliability are compared bit for
 * bit as u64, hops as integers; a pair is changed when any of the three differs.  kind bits:
 *   1  latency rose (lat1 > lat0)
 *   2  latency fell (lat1 < lat0; possible because any two topologies with the same attached
 *      vertices are accepted, not only parent and child)
 *   4  reliability bits differ
 *   8  hops differ
 * a's values are lat0 / rel0 / hops0, b's lat1 / rel1 / hops1.  Records come out in row-major
 * order, by srcCol then dstCol: deterministic.  Returns the total number of changed pairs; out
 * receives the first min(total, cap) records of that order (cap = 0 with out = NULL sizes the
 * buffer).  kindCount[i] = pairs with bit 1 << i set; rowChanged[s] = changed pairs of row s;
 * rowWorstRise[s] = the largest lat1 - lat0 (one f64 subtraction) over the pairs of row s whose
 * latency rose, rowWorstCol[s] the lowest column reaching it; 0.0 and -1 when no latency of the
 * row rises.  The three row arrays have A entries.  Any output pointer may be NULL.
 *
 * A topology without a valid table gets it built, as by shdtopo_build.  The call then takes both
 * build locks in a fixed order (by address).  Negative on an error: -1 NULL topology, negative
 * cap, or NULL out with cap > 0; -4 the attached vertex lists are not identical; -6 the two tables
 * live on different devices; -5 the attached sets kept changing under the call.  a == b is valid
 * and returns 0.
 *
 * Device work (topo_diff.hip): a count pass over the pairs, the exclusive scan of the row counts,
 * a fill pass that writes each row's records at its offset in column order (wave ballots and
 * prefix popcounts, no sort); 36 B are read per pair and pass, the fill pass skips rows without a
 * change and rows past cap.  Only the changed records and the per-row arrays leave the device.
 * Like the rest of the family the call materialises no lazy row, pushes no minimum, and leaves
 * ShdStats and the trace, load, crossings and timeline statistics as they were (a table it had to
 * build is a build like any other).  shdtopo_table_diff_stats reads the statistics of the last
 * diff in which `a` was the first argument. */
typedef struct {
    int32_t  srcCol, dstCol;
    double   lat0, lat1, rel0, rel1;
    uint16_t hops0, hops1;
    uint32_t kind;
} ShdTableChange;

typedef struct {
    double  total_ms;    /* wall time of the call (table builds it had to wait for included) */
    double  kernel_ms;   /* event time of count, scan and fill */
    int64_t pairs;       /* A x A */
    int64_t changed;     /* the call's return value */
    int64_t bytes_read;  /* table bytes the two passes read: 36 per pair of the count pass and of
                            every row the fill pass walked */
} ShdDiffStats;

int64_t shdtopo_table_diff(Topology* a, Topology* b, ShdTableChange* out, int64_t cap,
                           uint64_t kindCount[4], uint32_t* rowChanged /* [A] */,
                           double* rowWorstRise /* [A] */, int32_t* rowWorstCol /* [A] */);
int shdtopo_table_diff_stats(Topology* a, ShdDiffStats* out);

/* ---- flow impact: what a link failure does to a set of flows ----
 * shdtopo_table_diff answers "which attached pairs change"; shdtopo_flow_impact answers it for
 * traffic: n flows (source, destination, weight) are joined with the two device-resident tables of
 * a and b on the device -- four random gathers per flow -- and only the changed flows, integer
 * totals, a histogram of the delay rises and two per-column arrays leave it.
 *
 * Flows.  The host variant takes IPs and resolves them through a's map, as the trace and the load
 * do (an end that is not on a vertex of the current attached set is unattached); weight NULL means
 * 1 per flow.  The device variant takes the column arrays shdtopo_route_batch_device and
 * shdtopo_monitor_feed_device take (a column outside [0, A) is unattached) and a u32 payload as
 * the weight (NULL: 1 each); its kernels run on `stream` (NULL: a's own) behind whatever the
 * caller enqueued there, and the call returns when they are done.  n <= 2^31 - 2.
 *
 * Comparison.  Flow i is compared when both ends are columns.  A compared flow is changed exactly
 * when shdtopo_table_diff(a, b) would report its (srcCol, dstCol) pair: latency bits, reliability
 * bits or hops differ; kind is that call's kind.  a's values are lat0 / rel0 / hops0, b's lat1 /
 * rel1 / hops1.  Duplicate flows are separate flows.  Returns the number of changed flows; out
 * receives the first min(total, cap) records in ascending flow order (cap = 0 with out = NULL
 * sizes the buffer), nothing at or beyond cap is touched, and every other output is complete
 * whatever cap is.  Any output pointer may be NULL.
 *
 * Sums.  Every sum is a u64 that wraps, so no output depends on flow order, tiling or scheduling;
 * there is no floating-point sum.  delay = (uint64_t)ceil(lat * 1000000.0), the packet route's
 * delay in ns, and a flow's rise or fall is the difference of its two delays.  The histogram
 * covers the flows with kind & 1 by delay1 - delay0: a flow's bin is the number of edges <= its
 * rise, so bin 0 holds the rises below riseEdgeNs[0], bin nb those at or above the last edge, and
 * a rise equal to an edge goes to the upper bin; riseCount / riseWeight have nb + 1 entries,
 * 0 <= nb <= 1024, nb = 0 gives one bin.  srcChangedWeight[c] / dstChangedWeight[c] (A entries)
 * hold the weight of the changed flows that leave / enter column c.
 *
 * Errors, locks and side effects follow shdtopo_table_diff: -1 bad arguments (a NULL topology,
 * n < 0 or too large, a NULL end array with n > 0, cap < 0, NULL out with cap > 0, nb outside
 * [0, 1024], a NULL edge array with nb > 0, edges not strictly ascending); -4 the attached vertex
 * lists differ; -6 the tables are on different devices; -5 the attached sets kept moving.
 * Argument errors and -4 are returned before any device is used.  Missing tables are built as by
 * shdtopo_build, then both build locks are taken, the lower address first.  The call materialises
 * no lazy row, pushes no minimum and leaves ShdStats, the family's statistics and ShdDiffStats as
 * they were; its timing events are its own.  a == b is valid and answered without a table: the
 * flows are resolved (the device variant copies the columns and the payload to the host),
 * compared, unattached and weight are filled, everything else is zero, worstFlow is -1 and the
 * call returns 0.
 *
 * Device work (topo_impact.hip).  A count pass over tiles of 256 x U flows (tile_flows of the
 * statistics) gathers {lat, rel} and hops from both tables, keeps one ballot word per 64 flows,
 * reduces the totals in registers and LDS and numbers the tiles' changed flows; an exclusive scan
 * places the tiles; a fill pass gathers again only for the words that have a changed flow below
 * cap and writes the 48-B records at their ranks: flow order with no sort and no atomic.
 * shdtopo_flow_impact_stats reads the statistics of the last call in which `a` was the first
 * argument.  bytes_model, per flow: the count pass reads 8 B of columns and the weight (8 B, 4 B
 * or none), and for a compared flow two 16-B records and two 2-B hops (36 B); it writes one 8-B
 * word per 64 flows; the fill pass reads 8 B of columns and 36 B of table and writes 48 B for
 * every record it writes. */
typedef struct {            /* 48 B: three 16-B stores on the device */
    int64_t  flow;          /* request index i */
    double   lat0, lat1, rel0, rel1;
    uint16_t hops0, hops1;
    uint32_t kind;          /* shdtopo_table_diff's kind bits: 1 rose, 2 fell, 4 rel, 8 hops */
} ShdFlowChange;

typedef struct {
    int64_t  flows, compared, unattached, changed;
    uint64_t weight, changedWeight;          /* sums over compared / changed flows */
    uint64_t kindCount[4], kindWeight[4];
    uint64_t delayRiseNs, delayFallNs;       /* sum of w * |delay1 - delay0| over kind & 1 / kind & 2 */
    uint64_t hopsRise, hopsFall;             /* sum of w * |hops1 - hops0| over hops1 > hops0 / hops1 < hops0 */
    double   worstRise;                      /* max lat1 - lat0 (one f64 subtraction) over kind & 1; 0.0 if none */
    int64_t  worstFlow;                      /* the lowest flow index reaching it; -1 if none */
} ShdImpactTotals;

typedef struct {
    double  total_ms;       /* wall time of the call (table builds it had to wait for included) */
    double  resolve_ms;     /* of it: resolving the IPs to columns on the host (device variant: 0) */
    double  kernel_ms;      /* event time of count and scan, plus fill_ms */
    double  fill_ms;        /* event time of the fill pass (0: no record was asked for) */
    int64_t flows;          /* n */
    int64_t changed;        /* the call's return value */
    int64_t words_skipped;  /* 64-flow words (of (n + 63) / 64) the fill pass did not gather for */
    int64_t bytes_model;    /* the per-flow byte model above, summed over the call */
    int64_t tile_flows;     /* flows per workgroup of this build: 256 x U */
} ShdImpactStats;

int64_t shdtopo_flow_impact(Topology* a, Topology* b, const uint32_t* srcIP, const uint32_t* dstIP,
                            const uint64_t* weight /* NULL: 1 each */, int64_t n,
                            const uint64_t* riseEdgeNs, int64_t nb, ShdFlowChange* out,
                            int64_t cap, ShdImpactTotals* totals, uint64_t* riseCount,
                            uint64_t* riseWeight /* u64[nb + 1] each */,
                            uint64_t* srcChangedWeight, uint64_t* dstChangedWeight /* u64[A] each */);
int64_t shdtopo_flow_impact_device(Topology* a, Topology* b, const int32_t* d_srcCol,
                                   const int32_t* d_dstCol,
                                   const uint32_t* d_payload /* NULL: 1 each */, int64_t n,
                                   const uint64_t* riseEdgeNs, int64_t nb, ShdFlowChange* out,
                                   int64_t cap, ShdImpactTotals* totals, uint64_t* riseCount,
                                   uint64_t* riseWeight, uint64_t* srcChangedWeight,
                                   uint64_t* dstChangedWeight, void* stream);
int shdtopo_flow_impact_stats(Topology* a, ShdImpactStats* out);

/* ---- load shift: where a link failure moves a set of flows' traffic ----
 * shdtopo_flow_impact answers "which of my flows change"; shdtopo_load_shift answers where their
 * traffic goes: n flows (source host, destination host, weight -- the inputs of shdtopo_link_load)
 * are accumulated on a and on b, each by that topology's own load path and options ("load_walk",
 * "trace_batch", "trace_chunk"), both results stay on the device, are brought into the root
 * topology's numbering -- the numbering of shdtopo_edge_origin -- and compared entry by entry
 * there.  Only the entries whose load differs, and integer totals, leave the device.
 *
 * Index space.  R = the root's edge count, V = the vertex count.  Entry x in [0, 2 R + V) is
 *   x < R         the forward half of root edge x       (edgeLoad[e] of shdtopo_link_load),
 *   R <= x < 2 R  the reverse half of root edge x - R   (edgeLoad[E + e]),
 *   x >= 2 R      vertex x - 2 R                        (vertexLoad).
 * before(x) is a's load and after(x) is b's; an edge a topology lacks carries 0 there.  An entry
 * is changed exactly when before != after, compared as u64: a failed edge that carried nothing is
 * not reported.  Returns the number of changed entries; out receives the first min(total, cap)
 * records in ascending x (cap = 0 with out = NULL sizes the buffer), nothing at or beyond cap is
 * touched, and totals (may be NULL) is complete whatever cap is.
 *
 * Sums are u64 and wrap, comparisons are unsigned, there is no float anywhere: no output depends
 * on flow order, chunking, tiling or scheduling.
 *
 * Flows are resolved once, through a's map, as shdtopo_flow_impact does (vertex ids are common to
 * both topologies).  a and b may be parent and child, child and parent, two siblings, a topology
 * and a derivation of a derivation, or two loads of one file: beyond the checks below, edge
 * identity is the caller's word, as column identity is for shdtopo_table_diff.  Errors: -1 bad
 * arguments (a NULL topology, n < 0 or n > 2^31 - 2, a NULL IP array with n > 0, cap < 0, NULL out
 * with cap > 0); -7 the vertex counts or the root edge counts differ; -4 the attached vertex lists
 * differ; -6 the two topologies run their loads on different devices.  Argument errors, -7 and -4
 * are returned before any device is used.  Both build locks are taken, the lower address first,
 * for the whole call.  No table is needed, built or invalidated; like shdtopo_link_load the call
 * materialises no lazy row, pushes no minimum and leaves ShdStats and every other statistic of the
 * family -- both topologies' ShdLoadStats included -- exactly as it was.  a == b is valid: one
 * accumulation serves both sides and the call returns 0 with the totals of that load.  A complete
 * topology is accumulated on the host as shdtopo_link_load does and its sums are uploaded; when
 * both sides are complete the whole answer is computed on the host and no device is used.
 *
 * Device work (topo_shift.hip).  Each side brings the ascending list of the root edge ids it lacks
 * (a handful after a link failure; nothing for a root topology), and its own id of root edge r is
 * r - (the listed ids below r).  A count pass over tiles of 256 x U entries (tile_entries of the
 * statistics) loads both sides, keeps one ballot word per 64 entries, reduces the totals in
 * registers and LDS and numbers the tiles' changed entries; one workgroup merges the tiles'
 * {largest, lowest x} pairs; an exclusive scan places the tiles; a fill pass loads again only for
 * the words that have a changed entry below cap and writes the 32-B records at their ranks:
 * ascending x with no sort and no atomic.  shdtopo_load_shift_stats reads the statistics of the
 * last call in which `a` was the first argument.  bytes_model: the count pass reads 8 B per side
 * and entry the side has and writes one 8-B word per 64 entries and 72 B per tile; the fill pass
 * reads 16 B and writes 32 B for every record it writes. */
typedef struct {            /* 32 B: two 16-B stores on the device */
    int32_t  kind;          /* 0 forward half, 1 reverse half, 2 vertex */
    int32_t  id;            /* root edge id, or vertex id */
    int32_t  idA, idB;      /* the edge's id in a / in b, -1: that topology lacks it; vertices: id */
    uint64_t before, after;
} ShdLoadChange;

typedef struct {
    int64_t  flows, unattached;
    int64_t  routedA, routedB, brokenA, brokenB;
    uint64_t hopWeightA, hopWeightB;             /* link_load's hop_weight on each side */
    int64_t  changed[3], gained[3], lost[3];     /* entries by kind; gained: after > before */
    int64_t  newlyUsed[3], abandoned[3];         /* before == 0 < after / after == 0 < before */
    uint64_t gainedWeight[3], lostWeight[3];     /* wrapping sums of after-before / before-after */
    uint64_t displaced, appeared;                /* sum of before over edge halves b lacks / of after over halves a lacks */
    uint64_t worstGain, worstLoss;               /* largest after-before / before-after; 0 if none */
    int64_t  worstGainIndex, worstLossIndex;     /* the lowest x reaching it; -1 if none */
    uint64_t peakBefore, peakAfter;              /* largest load over the edge halves (x < 2R) */
    int64_t  peakBeforeIndex, peakAfterIndex;    /* lowest x reaching it; -1 when all are 0 */
} ShdShiftTotals;

typedef struct {
    double  total_ms;       /* wall time of the call */
    double  resolve_ms;     /* of it: resolving the IPs to vertices on the host */
    double  load_a_ms;      /* of it: a's accumulation, wall time (a complete side: its upload included) */
    double  load_b_ms;      /* of it: b's (0 when a == b) */
    double  kernel_ms;      /* event time of the compare kernels only: count, reduce, scan, fill */
    int64_t entries;        /* 2 R + V */
    int64_t changed;        /* the call's return value */
    int64_t words_skipped;  /* 64-entry words (of (entries + 63) / 64) the fill pass did not load for */
    int64_t bytes_model;    /* the byte model above, summed over the call (0: answered on the host) */
    int64_t tile_entries;   /* entries per workgroup of this build: 256 x U */
    ShdLoadStats loadA, loadB;  /* each side's accumulation as shdtopo_link_load_stats would report
                                   it (total_ms: the side's wall time; loadB = loadA when a == b) */
} ShdShiftStats;

int64_t shdtopo_load_shift(Topology* a, Topology* b, const uint32_t* srcIP, const uint32_t* dstIP,
                           const uint64_t* weight /* NULL: 1 each */, int64_t n,
                           ShdLoadChange* out, int64_t cap, ShdShiftTotals* totals);
int shdtopo_load_shift_stats(Topology* a, ShdShiftStats* out);

/* Test hook: the device graph preparation (topo_prep.hip) read back -- perm
 * int32[V] (relabelled -> original vertex), rowptr u32[V+1], the adjacency columns u32[2E']
 * (relabelled ids, rows ascending by neighbour), pi f64[V] (= d(h0, .), relabelled ids) and the
 * h0-tree parents u32[V] (relabelled, ~0 = none).  Any pointer may be NULL (call with NULLs to
 * size col).  Prepares the graph if needed.  Returns 2E', or a negative error (-2: complete or
 * directed topology, which have no such CSR). */
int64_t shdtopo_export_csr(Topology* top, int32_t* perm, uint32_t* rowptr, uint32_t* col,
                           double* pot, uint32_t* treeParent);

/* Test hook: one array of the graph preparation or of the last build's target
 * preparation (4b) by name, copied to out (cap_bytes bytes).  Takes the build lock, prepares the
 * graph if needed and drains the library's stream first (the target preparation is enqueued
 * asynchronously).  Works for directed topologies.  Relabelled ids throughout.
 *   graph:    perm, inv i32[V]; rowptr u32[V+1]; adj u32[4] per entry (in-rows when directed);
 *             aloss f64 per entry; vloss, self_lat, self_loss, pot f64[V]; pi_max f64[1];
 *             spt_parent u32[V]; spt u32[8] per vertex; adjk u32[4], kap f32 per entry; ksum
 *             f32[probes] per vertex; kap0 f32[V]; kf_kap f64 per entry; hub_seg u32[2] per
 *             segment; hub_multi u32[4] per row cut in several
 *   directed: rowptr_in u32[V+1]; adj_out u32[4] per entry; pot_src f64[V]
 *   targets:  tbits, tbits_eff, dead u32[(V+31)/32]; tleaf u32[8] per target; kfix f64[2V], the
 *             final [K | Kt]
 *   state:    i32[8] {adjk plain, flagged, resorted, leaf, kappa probes, kappa0 in the records,
 *             hub segment length, grouping hubs}
 * Returns the bytes copied; with out == NULL the array's size in bytes; -1: unknown name; -2:
 * the array does not exist (complete topology, undirected topology's directed arrays, target
 * arrays not built in this state); -3: cap_bytes too small. */
int64_t shdtopo_export_prep(Topology* top, const char* name, void* out, int64_t cap_bytes);

/* Copy the parsed graph into host arrays (document order; any pointer may be NULL):
 * eu, ev int32[E]; elat, eloss f64[E]; vloss f64[V].  Used by tools and oracle cross-checks. */
int shdtopo_export_graph(Topology* top, int32_t* eu, int32_t* ev, double* elat, double* eloss,
                         double* vloss);

/* Write the loaded graph back out as GraphML (same key schema as the bundled resource files). */
int shdtopo_write_graphml(Topology* top, const char* path);

/* ---- synthetic workloads (BASELINE.json configs 4/5; tools, not on the routing path) ---- */
typedef struct {
    uint64_t seed;
    int64_t n_routers;   /* 990000 */
    int64_t n_poi;       /* 10000 */
    int64_t n_edges;     /* 10000000 undirected edges in total, incl. poi uplinks + self loops */
    int integer_latency; /* 1: latency ~ U{1..100} (heavy ties) */
    double alpha;        /* Chung-Lu endpoint weight ~ rank^(-alpha); 1/1.1 */
    int directed;        /* 1: a directed topology -- every non-loop edge becomes two arcs, the
                            reverse one with its own latency and loss draw (uplinks 5.0 both
                            ways), so E = 2 x n_edges - n_poi (tools: directed-path probes) */
} ShdSynthParams;
Topology* shdtopo_new_synthetic(const ShdSynthParams* p);

/* Attach n_hosts hosts with Tor-like type hints (94 % client, 5 % relay, 1 % server) following
 * Shadow's seed chain (master --seed -> slave seed -> per-host nodeSeed), IPs
 * 11.0.0.1 + k; host k < (number of poi with a usable ip) is pinned to the k-th poi by an exact
 * ipHint (so every poi of a synthetic topology is attached); then emit n_packets packets of one window: src uniform over hosts, dst by role,
 * payload 1448 w.p. 0.8 else 0, pre-draw rand_r state from each host's stream, now ~
 * U[t0, t0 + jump).  Output arrays are host memory of length n_packets (hostState: n_hosts,
 * the hosts' states after attach). */
int shdtopo_synth_packets(Topology* top, uint64_t seed, int64_t n_hosts, int64_t n_packets,
                          uint64_t t0, uint64_t jump, int32_t* srcCol, int32_t* dstCol,
                          uint32_t* payload, uint32_t* stateIn, uint64_t* now,
                          uint32_t* srcIP, uint32_t* dstIP);

/* ---- traffic matrix: packet windows summed into per-pair flows ----
 * Every analysis call of the family -- shdtopo_link_load, shdtopo_link_crossings,
 * shdtopo_link_timeline, shdtopo_flow_impact, shdtopo_load_shift -- takes a set of flows (source
 * host, destination host, weight).  A traffic matrix makes that set from a run: a persistent
 * object of its topology, fed like a link monitor, that sums packets and weight per (source
 * vertex, destination vertex) and exports its non-zero cells in order.  It needs no table, no
 * chains and no routes, only the column geometry.
 *
 * Layout.  The matrix owns an ascending list mv of M original vertex ids and M x M cells of 16 B,
 * {u64 packets, u64 weight}, row-major, row = source, column = destination.  mv starts empty.
 * Before counting anything every feed compares the current column geometry (the columns
 * shdtopo_route_batch_device sees, those deferred by shdtopo_window_hold included) with mv; if an
 * attached vertex is missing the matrix grows: mv' is the sorted union, new cells are allocated
 * and every old cell moves to its new place (a re-layout).  A vertex that later loses its column
 * keeps its row, its column and its totals for good.  If 16 M'^2 bytes exceed option "matrix_mb"
 * (a double, MB; 0, the default: half of the device memory free at that growth, no cap for host
 * cells) the growth and the feed return -5 -- tested before anything is allocated; nothing is
 * counted and the matrix, with its old mv, is untouched.
 *
 * A complete topology's host feeds accumulate in host cells and initialise no device; its device
 * feeds use device cells.  Every other topology stages its host arrays and runs the feed kernel.
 * A read that finds only host cells is answered on the host; one that finds both first adds the
 * host cells into the device cells and clears them.
 *
 * Every sum is a u64 that wraps.  No output depends on the order of the feeds, on how the packets
 * are split into feeds, on tiling or on scheduling.
 *
 * Matrices are small integer ids of their topology, as monitors are: a stale id or another
 * topology's id returns -1 from every call and dereferences nothing; shdtopo_topology_free
 * releases what is left.
 *
 *   shdtopo_matrix_new       id >= 0; uses no device.
 *   shdtopo_matrix_feed      host arrays; the IPs resolve as in shdtopo_monitor_feed (an end that
 *                            is no column: unattached, skipped and counted).  Packets with
 *                            delivered[i] == 0 are skipped and counted.  Each remaining packet
 *                            adds 1 to packets and weight[i] (NULL: 1) to weight of its cell; a
 *                            self pair goes to the diagonal.  Returns the packets this feed
 *                            counted.  -1: a NULL end array with n > 0, n < 0 or n > 2^31 - 2.
 *   shdtopo_matrix_feed_vertices  the same with original vertex ids (-1 = not attached).
 *   shdtopo_matrix_feed_device    the arrays of shdtopo_route_batch_device, resident in device
 *                            memory; enqueued on `stream` (NULL: the library's), not awaited;
 *                            returns 0 or a negative error.  A column outside [0, A) is skipped
 *                            and counted (bad_columns), nothing is read through it.  The matrix
 *                            owns one event: each device feed records it on its stream, a feed on
 *                            another stream than the previous one first waits on it.
 *   shdtopo_matrix_vertices  mv (the first min(M, cap) entries; out may be NULL); returns M.
 *   shdtopo_matrix_read      the reported cells -- those with packets != 0 || weight != 0 -- as
 *                            ShdMatrixFlow records in ascending (srcVertex, dstVertex) order;
 *                            returns their number.  out gets the first min(total, cap) of them,
 *                            nothing at or beyond cap is touched; cap = 0 with out = NULL sizes
 *                            the buffer.  Every other output is complete whatever cap is; any
 *                            output pointer may be NULL.  sent* are the row sums, recv* the column
 *                            sums over all cells (u64[M] each).
 *   shdtopo_matrix_reset     zeroes the cells and the cumulative counters; keeps mv.
 *   shdtopo_matrix_stats     counters and sizes, below.
 *   shdtopo_vertex_ips       per vertex the attached IP (network order) that is lowest when read
 *                            in host byte order, 0 when no host is on it; returns the vertices
 *                            that got one, -1 for bad arguments or a vertex outside [0, V).  Host
 *                            only.  It turns exported cells into flows the rest of the family
 *                            accepts: routes depend on the vertex alone, so any host of the
 *                            vertex stands for it.
 * read, stats, reset, vertices and free synchronise the matrix's event and the library's stream
 * first.  The n == 0 feed launches nothing.
 *
 * Every call takes the build lock; none materialises a lazy row, pushes a minimum, builds or
 * invalidates a table; each leaves ShdStats and every other statistic of the family as it was.
 * A multi-device topology uses its first device. */
typedef struct {
    int32_t  srcVertex, dstVertex;  /* original vertex ids */
    int32_t  srcIndex, dstIndex;    /* their places in mv */
    uint64_t packets, weight;
} ShdMatrixFlow;

typedef struct {
    int64_t  size;                  /* M */
    int64_t  cells;                 /* reported cells */
    uint64_t packets, weight;       /* over all cells */
    int64_t  selfCells;             /* reported cells on the diagonal */
    uint64_t selfPackets, selfWeight;
    int64_t  activeSources;         /* rows with a reported cell */
    int64_t  activeDestinations;    /* columns with a reported cell */
    uint64_t peakWeight;            /* the largest weight of a reported cell (0: none) */
    int64_t  peakCell;              /* the lowest i * M + j reaching it; -1: no reported cell */
} ShdMatrixTotals;

typedef struct {
    double  feed_kernel_ms;         /* event time of the last feed's kernel (0: none, host cells) */
    double  read_ms;                /* wall time of the last read */
    double  read_kernel_ms;         /* of it: event time of the count, scan and fill passes */
    double  relayout_ms;            /* wall time of the last growth */
    /* cumulative since matrix_new / matrix_reset */
    int64_t fed;                    /* packets counted */
    int64_t skipped_undelivered;    /* delivered[i] == 0 */
    int64_t unattached;             /* host feeds: an end that is no column */
    int64_t bad_columns;            /* device feeds: a column outside [0, A) */
    /* the last feed alone */
    int64_t last_fed, last_skipped_undelivered, last_unattached, last_bad_columns;
    int64_t feeds;                  /* feed calls since matrix_new */
    int64_t size;                   /* M */
    int64_t bytes;                  /* 16 M^2 */
    int64_t relayouts;              /* growths that moved cells (an empty matrix moves none) */
    int64_t cells;                  /* reported cells of the last read */
    int64_t bytes_model;            /* the last read's modelled traffic: 16 M^2 (count) + 16 M per
                                       row the fill walked + 32 per record written; a feed's
                                       model is 8 B of columns + the weight (4, 8 or 0) + 1 B of
                                       delivered per packet and two atomics on one 16-B cell */
} ShdMatrixStats;

int shdtopo_matrix_new(Topology* top);
int shdtopo_matrix_free(Topology* top, int id);
int64_t shdtopo_matrix_feed(Topology* top, int id, const uint32_t* srcIP, const uint32_t* dstIP,
                            const uint64_t* weight /* NULL: 1 each */,
                            const uint8_t* delivered /* NULL: all */, int64_t n);
int64_t shdtopo_matrix_feed_vertices(Topology* top, int id, const int32_t* srcVertex,
                                     const int32_t* dstVertex, const uint64_t* weight,
                                     const uint8_t* delivered, int64_t n);
int shdtopo_matrix_feed_device(Topology* top, int id, const int32_t* d_srcCol,
                               const int32_t* d_dstCol,
                               const uint32_t* d_payload /* weight; NULL: 1 each */,
                               const uint8_t* d_delivered /* NULL: all */, int64_t n,
                               void* stream);
int64_t shdtopo_matrix_vertices(Topology* top, int id, int32_t* out, int64_t cap);
int64_t shdtopo_matrix_read(Topology* top, int id, ShdMatrixFlow* out, int64_t cap,
                            uint64_t* sentPackets, uint64_t* sentWeight, uint64_t* recvPackets,
                            uint64_t* recvWeight /* u64[M] each; may be NULL */,
                            ShdMatrixTotals* totals /* may be NULL */);
int shdtopo_matrix_reset(Topology* top, int id);
int shdtopo_matrix_stats(Topology* top, int id, ShdMatrixStats* out);
int64_t shdtopo_vertex_ips(Topology* top, const int32_t* vertex, int64_t n, uint32_t* ip);

/* ---- route schedule: packets routed by the topology live at their emit time ----
 * The what-if family compares a topology with a derived one offline; a schedule puts the two into
 * one run: a link fails at t = 40 s and comes back at t = 70 s.  A schedule is k topologies
 * tops[0..k) with start times fromNs[0..k): 1 <= k <= SHD_SCHEDULE_MAX, fromNs[0] == 0, fromNs
 * strictly ascending.  The same topology may appear in several epochs ([parent, child, parent]).
 * Every member must have the same attached vertices as tops[0] (a derived topology carries its
 * parent's hosts), so a column means the same host vertex in every table.
 *
 * Semantics.  Packet i belongs to epoch e(i), the largest e with fromNs[e] <= now[i], and its
 * outputs (time, rngState, delivered) are bit for bit what shdtopo_route_batch_device on
 * tops[e(i)] alone returns for it: the {lat, rel} gather at [srcCol][dstCol], the rand_r steps and
 * the chance <= rel || payload == 0 rule, the (uint64_t)ceil(lat * 1000000.0) delay, the clamp; a
 * column outside [0, A) gives delivered 0, time 0 and the state unchanged.  The route is decided
 * at emission, as worker_schedulePacket decides it: a packet emitted before a failure and
 * arriving after it is delivered.  The schedule always reads the forward row [src][dst] of each
 * table, like the device route: it emulates no lazy orientation, materialises no lazy row, pushes
 * no minimum and leaves ShdStats and every family statistic as they were (its counters and timing
 * events are its own).  A table it had to build counts as a build like any other.
 *
 * Outputs.  d_epoch / epoch (may be NULL) receives e(i), one byte per packet.  epochCount (host
 * u64[k][3], may be NULL): {packets of epoch e, of them delivered, of them not routed}, exact
 * counts reduced on the device, independent of tiling; a packet that is not routed still has an
 * epoch, taken from its now.
 *
 * Variants.  The device variant takes the arrays of shdtopo_route_batch_device and runs its
 * kernel on `stream` (NULL: tops[0]'s own) behind whatever is enqueued there; it returns when the
 * kernel is done, so the tables stay locked while they are read, and returns 0.  The host
 * variants resolve vertices (and IPs) through tops[0], with shdtopo_route_batch_vertices' rule for
 * a vertex that is no column: the packet is not routed -- delivered 0, time 0, rngState the state
 * after its one draw -- and they return the number of such packets.  n = 0 with valid arguments
 * returns 0 and builds nothing.
 *
 * Errors: -1 bad arguments (NULL tops or a NULL member, k outside [1, 16], fromNs[0] != 0, fromNs
 * not strictly ascending, n < 0, a NULL array with n > 0); -4 the members' attached vertex lists
 * are not all identical; -6 the tables are not all on one device; -5 the attached sets kept
 * changing under the call.  Argument errors and -4 are returned before any device is used.
 * Missing tables are built as by shdtopo_build, then the build locks of the distinct members are
 * taken in address order.  A multi-device member is read on its first device.
 *
 * Device work (topo_schedule.hip): packet_route_kernel's tile with the k table pointers and start
 * times passed by value; 53 B per packet as the one-table route (24 B in, a 16-B gather, 13 B
 * out), plus 1 B with d_epoch.  shdtopo_route_schedule_stats reads the statistics of the last
 * call whose tops[0] was `first`. */
#define SHD_SCHEDULE_MAX 16
typedef struct {
    double  total_ms;       /* wall time of the call (table builds it had to wait for included) */
    double  kernel_ms;      /* event time of the kernel (events of the call's own) */
    int64_t packets;        /* n */
    int64_t epochs;         /* k */
    int64_t not_routed;     /* packets with a column outside [0, A) / a vertex that is no column */
    int64_t epoch_packets[SHD_SCHEDULE_MAX];
    int64_t epoch_delivered[SHD_SCHEDULE_MAX];
    int64_t bytes_model;    /* 53 B per packet, 54 with the epoch output */
} ShdScheduleStats;

int64_t shdtopo_route_schedule_device(Topology* const* tops, const uint64_t* fromNs, int k,
                                      const int32_t* d_srcCol, const int32_t* d_dstCol,
                                      const uint32_t* d_payload, const uint32_t* d_stateIn,
                                      const uint64_t* d_now, int64_t n, uint64_t jumpNs, int clamp,
                                      uint64_t* d_time, uint32_t* d_stateOut, uint8_t* d_delivered,
                                      uint8_t* d_epoch /* may be NULL */,
                                      uint64_t* epochCount /* host u64[k][3], may be NULL */,
                                      void* stream);
int64_t shdtopo_route_schedule_vertices(Topology* const* tops, const uint64_t* fromNs, int k,
                                        const int32_t* srcVertex, const int32_t* dstVertex,
                                        const uint32_t* payloadLength, const uint32_t* rngState,
                                        const uint64_t* now, int64_t n, uint64_t jumpNs,
                                        int clampInterHost, TopoPacketOut* out,
                                        uint8_t* epoch /* host, may be NULL */,
                                        uint64_t* epochCount);
int64_t shdtopo_route_schedule(Topology* const* tops, const uint64_t* fromNs, int k,
                               const TopoPacketIn* in, TopoPacketOut* out, int64_t n,
                               uint64_t jumpNs, int clampInterHost, uint8_t* epoch,
                               uint64_t* epochCount);
int shdtopo_route_schedule_stats(Topology* first, ShdScheduleStats* out);

#ifdef __cplusplus
}
#endif
#endif /* SHD_TOPOLOGY_ABI_H_ */
