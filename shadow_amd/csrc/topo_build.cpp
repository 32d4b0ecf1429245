// topo_build.cpp -- the whole-table build behind ensure_table / shdtopo_build_rows (topo_core.cpp):
// the batch layout and its measured costs, enqueue_rows as a sequence of stages (each names the HIP
// calls it enqueues and where the host blocks), collect_row_stats, and the multi-GPU build with its
// RCCL loader and peer copies.
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "topo_host.h"

namespace shdtopo {

// sample rows of the tie probe (tie_probe): 8 batches of 8, one short launch
constexpr int64_t kTieProbeRows = 64;

// The batch layout of a launch goes to the device: output row (rowmap) and source of each
// position, its bucket shift sh = C - d(src, h0) >= 2 delta (every source's h0 at C, h0_shift;
// topo_sssp_batch.hip), and the batch starts of a measured layout.
int upload_layout(Topology* top, const std::vector<uint32_t>& src, const std::vector<uint32_t>& perm,
                  const std::vector<uint32_t>* bstart, double delta, hipStream_t st) {
    const int64_t rows = (int64_t)src.size();
    std::vector<uint32_t>& psrc = top->layPsrc;
    psrc.resize((size_t)rows);
    for (int64_t i = 0; i < rows; i++) psrc[(size_t)i] = src[(size_t)perm[(size_t)i]];
    HIPCHK(top->d_rowmap.ensure((size_t)rows));
    HIPCHK(top->d_bsrc.ensure((size_t)rows));
    HIPCHK(hipMemcpyAsync(top->d_rowmap.p, perm.data(), 4 * (size_t)rows, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(top->d_bsrc.p, psrc.data(), 4 * (size_t)rows, hipMemcpyHostToDevice, st));
    const std::vector<double> sh = source_shifts(top, psrc.data(), rows, delta);
    HIPCHK(top->d_srcsh.ensure((size_t)rows));
    HIPCHK(hipMemcpyAsync(top->d_srcsh.p, sh.data(), sizeof(double) * (size_t)rows,
                          hipMemcpyHostToDevice, st));
    const std::vector<double> hs = source_h0_seeds(top, psrc.data(), rows);
    HIPCHK(top->d_h0seed.ensure((size_t)rows));
    HIPCHK(hipMemcpyAsync(top->d_h0seed.p, hs.data(), sizeof(double) * (size_t)rows,
                          hipMemcpyHostToDevice, st));
    if (bstart) {
        HIPCHK(top->d_bstart.ensure(bstart->size()));
        HIPCHK(hipMemcpyAsync(top->d_bstart.p, bstart->data(), 4 * bstart->size(),
                              hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // perm / sh / hs / bstart must outlive the copies
    return 0;
}

// the kernel's contract (topo_sssp_batch.hip): runs of 1..K positions covering [0, rows)
static bool check_runs(const std::vector<uint32_t>& lstart, int64_t rows, int K) {
    if (lstart.size() < 2 || lstart.front() != 0u || lstart.back() != (uint32_t)rows) return false;
    for (size_t b = 0; b + 1 < lstart.size(); b++)
        if (lstart[b + 1] <= lstart[b] || lstart[b + 1] - lstart[b] > (uint32_t)K) return false;
    return true;
}

// Measured batch layout (option balance).  A batch's wall time is modelled
// as a fixed part a plus its sources' costs; both come from the batch times of earlier launches
// on this graph (record_costs).  Once every source of the rows has a cost:
//  * one round of the slots (an 8-GPU shard): the grouping order (source_order) is cut into at
//    most `slots` runs of <= K consecutive positions minimising the largest predicted batch
//    (greedy cuts under a bisected bound) -- batches stay runs of the grouping, so the sources
//    that share expansions stay together, but a run of expensive sources gets fewer of them;
//  * several rounds: batches of kf in the grouping order, dequeued longest predicted first (the
//    dynamic dequeue is then list scheduling in LPT order), the ragged batch last.
// The layout changes only which batch computes a row: every row is the same (bit-exact tests).
// A re-cut from the updated costs each build beat refining the previous cut (moving edge sources
// off the slowest batches): a batch's time repeats within ~0.3 ms for the same sources but is
// predicted from other compositions only loosely (corr 0.4-0.7), and both end near 11 ms at 1,250
// rows.
// The layout from the costs c (per position of the grouping order) and the fixed part a: `order`
// lists the grouping positions in launch order, `lstart` the batch starts (shdtopo_test_batch_layout
// exposes it to the CPU tests).
bool layout_from_costs(const std::vector<double>& c, double a, int kf, int slots, int K,
                       std::vector<uint32_t>& order, std::vector<uint32_t>& lstart) {
    const int64_t rows = (int64_t)c.size();
    if (rows < 1 || kf < 1 || kf > K || slots < 1) return false;
    const int64_t nplain = (rows + kf - 1) / kf;
    order.resize((size_t)rows);
    std::iota(order.begin(), order.end(), 0u);
    lstart.clear();
    if (nplain <= (int64_t)slots) {
        // the fewest runs whose predicted cost stays <= B (greedy is optimal for a bound)
        auto cut = [&](double B, std::vector<uint32_t>* out) -> int64_t {
            int64_t n = 0, i = 0;
            if (out) out->push_back(0u);
            while (i < rows) {
                double s = a;
                int m = 0;
                while (i < rows && m < K && (m == 0 || s + c[(size_t)i] <= B)) {
                    s += c[(size_t)i];
                    i++;
                    m++;
                }
                n++;
                if (out) out->push_back((uint32_t)i);
            }
            return n;
        };
        double lo = a, hi = a;
        for (int64_t b = 0; b < nplain; b++) {  // the plain layout's largest batch: feasible
            double s = a;
            for (int64_t i = b * kf; i < std::min(rows, (b + 1) * kf); i++) s += c[(size_t)i];
            hi = std::max(hi, s);
        }
        for (int64_t i = 0; i < rows; i++) lo = std::max(lo, a + c[(size_t)i]);
        if (cut(hi, nullptr) > (int64_t)slots) return false;
        for (int it = 0; it < 40 && hi - lo > 1e-4 * hi; it++) {
            const double mid = 0.5 * (lo + hi);
            if (cut(mid, nullptr) <= (int64_t)slots) hi = mid;
            else lo = mid;
        }
        cut(hi, &lstart);
    } else {
        std::vector<double> bc((size_t)nplain, a);
        for (int64_t i = 0; i < rows; i++) bc[(size_t)(i / kf)] += c[(size_t)i];
        std::vector<uint32_t> bo((size_t)nplain);
        std::iota(bo.begin(), bo.end(), 0u);
        const bool ragged = rows % kf != 0;
        std::stable_sort(bo.begin(), bo.end() - (ragged ? 1 : 0),
                         [&](uint32_t x, uint32_t y) { return bc[x] > bc[y]; });
        order.clear();
        lstart.push_back(0u);
        for (uint32_t b : bo) {
            for (int64_t i = (int64_t)b * kf; i < std::min(rows, ((int64_t)b + 1) * kf); i++)
                order.push_back((uint32_t)i);
            lstart.push_back((uint32_t)order.size());
        }
    }
    return check_runs(lstart, rows, K);
}

bool measured_layout(Topology* top, const std::vector<uint32_t>& src, int kf, int slots,
                     std::vector<uint32_t>& lperm, std::vector<uint32_t>& lstart) {
    const int64_t rows = (int64_t)src.size();
    const std::vector<uint32_t>& base = top->ordBase;
    if (top->costHp != top->hp.get() || (int64_t)base.size() != rows || rows < 2) return false;
    std::vector<double> c((size_t)rows);
    for (int64_t i = 0; i < rows; i++) {
        const float x = top->srcCost[(size_t)src[(size_t)base[(size_t)i]]];
        if (!(x > 0.0f)) return false;
        c[(size_t)i] = (double)x;
    }
    std::vector<uint32_t> order;
    if (!layout_from_costs(c, top->costA, kf, slots, batch_k(top), order, lstart)) return false;
    lperm.resize((size_t)rows);
    for (int64_t i = 0; i < rows; i++) lperm[(size_t)i] = base[(size_t)order[(size_t)i]];
    return true;
}

// Costs from a launch's batch times (SlotWs::btrace: dequeue and end ticks per batch): the
// fixed part a = 1/3 of the mean batch (C4: a lone source takes 4.3 ms, a batch of 5 8.9 ms,
// of 8 10.2 ms), the rest shared equally by the batch's sources; both averaged with the earlier
// builds' (weight 1/2), so a source that moves to another batch converges to its own share.
void record_costs(Topology* top, const std::vector<uint32_t>& psrc, const std::vector<uint32_t>& lstart,
                  const std::vector<unsigned long long>& bt) {
    const int64_t nb = (int64_t)lstart.size() - 1;
    if (nb < 1) return;
    if (top->balance == 2 && top->costHp == top->hp.get()) return;  // frozen (diagnostic)
    if (top->costHp != top->hp.get() || (int64_t)top->srcCost.size() != top->g.V) {
        top->srcCost.assign((size_t)top->g.V, 0.0f);
        top->costHp = top->hp.get();
        top->costA = 0.0;
    }
    std::vector<double> T((size_t)nb, 0.0);
    double sum = 0.0;
    int64_t n = 0;
    for (int64_t b = 0; b < nb; b++) {
        const unsigned long long t0 = bt[(size_t)b * kBTraceWords], t1 = bt[(size_t)b * kBTraceWords + 1];
        if (t1 > t0) {
            T[(size_t)b] = (double)(t1 - t0);
            sum += T[(size_t)b];
            n++;
        }
    }
    if (n == 0) return;
    const double mean = sum / (double)n, a = mean / 3.0;
    top->costA = top->costA > 0.0 ? 0.5 * (top->costA + a) : a;
    for (int64_t b = 0; b < nb; b++) {
        if (!(T[(size_t)b] > 0.0)) continue;
        const uint32_t p0 = lstart[(size_t)b], p1 = lstart[(size_t)b + 1];
        const double cs = std::max(0.01 * mean, (T[(size_t)b] - a) / (double)(p1 - p0));
        for (uint32_t p = p0; p < p1 && p < psrc.size(); p++) {
            float& x = top->srcCost[(size_t)psrc[p]];
            x = x > 0.0f ? (float)(0.5 * ((double)x + cs)) : (float)cs;
        }
    }
}

// wall checkpoints of a whole-table build (ShdStats.build_step_ms): the time since the previous
// mark goes to step i
void bstep_mark(Topology* top, int i) {
    const auto t = std::chrono::steady_clock::now();
    top->stats.build_step_ms[i] += std::chrono::duration<double, std::milli>(t - top->bstepT).count();
    top->bstepT = t;
}

// per-build cold-path timings start at 0: a build that finds the graph (or the target set)
// already prepared reports 0 for that step
void reset_build_stats(Topology* top) {
    top->stats.csr_ms = top->stats.csr_host_ms = top->stats.csr_copy_ms = 0.0;
    top->stats.order_ms = top->stats.replay_prep_ms = top->stats.target_prep_ms = 0.0;
    top->stats.batch_layout_measured = 0;
    top->lastBatches = 0;
    top->stats.workspace_ms = 0.0;
    top->stats.csr_host_runs = 0;
    top->stats.tie_probe_rows = top->stats.tie_probe_flagged = 0;
    top->stats.tie_probe_ms = 0.0;
}

// The target-aware re-sort's scratch for the prepared relaxation copy (allocated once).
// The long rows' entries for the segmented sort's device-wide radix sort (SegBig): positions
// row by row, each entry's row ordinal, and the sort's end bit.
void plan_long_rows(const uint32_t* rowptr, int64_t V, std::vector<uint32_t>& pos,
                    std::vector<uint32_t>& row, int* end_bit) {
    pos.clear();
    row.clear();
    uint32_t nrow = 0;
    for (int64_t v = 0; v < V; v++) {
        const uint32_t b = rowptr[v], e = rowptr[v + 1];
        if (e - b <= kSegBlock) continue;
        for (uint32_t p = b; p < e; p++) {
            pos.push_back(p);
            row.push_back(nrow);
        }
        nrow++;
    }
    int bits = 1;
    while (bits < 31 && (1u << bits) < nrow) bits++;
    *end_bit = 32 + bits;
}

int ensure_kprime_scratch(Topology* top, KprimeScratch* out) {
    const int64_t nadj = (int64_t)(top->d_adjk.n / 4), V = top->g.V;
    if (top->kpBig < 0) {
        // the long rows (the graph's rows never change: listed once, in the preparation)
        std::vector<uint32_t> rp((size_t)V + 1), pos, row;
        HIPCHK(hipMemcpyAsync(rp.data(), top->d_rowptr.p, 4 * ((size_t)V + 1), hipMemcpyDeviceToHost,
                              top->stream));
        HIPCHK(hipStreamSynchronize(top->stream));
        plan_long_rows(rp.data(), V, pos, row, &top->kpBigBits);
        const size_t nb = pos.size();
        HIPCHK(top->d_kpBigPos.ensure(std::max<size_t>(1, nb)));
        HIPCHK(top->d_kpBigRow.ensure(std::max<size_t>(1, nb)));
        HIPCHK(top->d_kpBigKey.ensure(std::max<size_t>(1, 2 * nb)));
        HIPCHK(top->d_kpBigVal.ensure(std::max<size_t>(1, 2 * nb)));
        if (nb) {
            HIPCHK(hipMemcpyAsync(top->d_kpBigPos.p, pos.data(), 4 * nb, hipMemcpyHostToDevice, top->stream));
            HIPCHK(hipMemcpyAsync(top->d_kpBigRow.p, row.data(), 4 * nb, hipMemcpyHostToDevice, top->stream));
            HIPCHK(hipStreamSynchronize(top->stream));
        }
        top->kpBig = (int64_t)nb;
    }
    size_t tb = 0;
    HIPCHK(segsort_big_tmp_bytes(top->kpBig, top->kpBigBits, &tb));
    const size_t n = (size_t)std::max<int64_t>(1, nadj);
    HIPCHK(top->d_kpKey.ensure(n));
    HIPCHK(top->d_kpIdx.ensure(n));
    HIPCHK(top->d_kpRec.ensure(n));
    HIPCHK(top->d_kpTmp.ensure(std::max<size_t>(1, tb)));
    if (out) {
        out->key = top->d_kpKey.p;
        out->idx = top->d_kpIdx.p;
        out->rec = top->d_kpRec.p;
        SegBig& b = out->big;
        b.pos = top->d_kpBigPos.p;
        b.row = top->d_kpBigRow.p;
        b.nitems = top->kpBig;
        b.end_bit = top->kpBigBits;
        b.keys = top->d_kpBigKey.p;
        b.vals = top->d_kpBigVal.p;
        b.tmp = top->d_kpTmp.p;
        b.tmp_bytes = top->d_kpTmp.n;
    }
    return 0;
}

namespace {

// What the stages of one enqueue_rows call share; lives for that call.
struct RowsCall {
    int64_t row0 = 0, rows = 0, A = 0;
    int K = 0;                       // sources per workgroup (batch_k)
    std::vector<uint32_t> src, tgt;  // relabelled ids: the rows' sources, the columns' targets
    double2* out_lr = nullptr;
    uint16_t* out_hops = nullptr;
    double* out_rowmin = nullptr;
    hipStream_t st = nullptr;
    SlotWs ws;  // the batched launches' view of the workspace: row flags, leaf records, layout
    // every row goes to the heap replay: tie-dense before the build (dense), that or replay_all or
    // a multigraph (allReplay), or the tie probe of this build found the topology tie-dense
    bool dense = false, allReplay = false, probeDense = false;
    int kf = 0;          // sources per batch of the batched launch (batch_fill_for)
    double delta = 0.0;  // ... and its bucket width
    // the batched launch's per-batch times, read back after its closing event: its batch
    // starts, fill (0: measured layout), slots and the SHD_BATCH_TRACE file
    struct {
        std::vector<uint32_t> start;
        int kf = 0, slots = 0;
        const char* file = nullptr;
    } bt;
};

// a build's device counters start over: all zero, the global minimum +inf
int reset_dev_stats(Topology* top, hipStream_t st) {
    HIPCHK(hipMemsetAsync(top->d_stats.p, 0, sizeof(unsigned long long) * ST_COUNT, st));
    HIPCHK(launch_fill_u64(top->d_stats.p + ST_GLOBAL_MIN, 0x7FF0000000000000ull, 1, st));
    return 0;
}

// the kernels' closing event; the host waits for the stream
int close_and_wait(Topology* top, hipStream_t st) {
    HIPCHK(hipEventRecord(top->ev1, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// Complete graph: the pair matrices (blocking uploads, when the columns changed), then ev0, one
// launch, ev1.
int enqueue_complete(Topology* top, RowsCall& c) {
    const int64_t A = c.A;
    hipStream_t st = c.st;
    // dense A x A direct-edge matrices (lowest edge id wins, as orc_get_eid), resident in HBM
    // while the columns stay: rebuilt only when the attached set changed
    if (top->aaCols != top->attached || !top->d_elatAA.p || !top->d_vlossA.p) {
        std::vector<double> elat((size_t)(A * A), -1.0), eloss((size_t)(A * A), 0.0), vl((size_t)A);
        const HostGraph& g = top->g;
        for (int64_t e = 0; e < g.E; e++) {
            int32_t ca = top->colOf[(size_t)g.eu[(size_t)e]], cb = top->colOf[(size_t)g.ev[(size_t)e]];
            if (ca < 0 || cb < 0) continue;
            auto put = [&](size_t k) {
                if (elat[k] < 0) { elat[k] = g.elat[(size_t)e]; eloss[k] = g.eloss[(size_t)e]; }
            };
            put((size_t)ca * (size_t)A + (size_t)cb);
            if (!g.directed) put((size_t)cb * (size_t)A + (size_t)ca);
        }
        for (int64_t i = 0; i < A; i++) vl[(size_t)i] = g.vloss[(size_t)top->attached[(size_t)i]];
        HIPCHK(top->d_elatAA.ensure((size_t)(A * A)));
        HIPCHK(top->d_elossAA.ensure((size_t)(A * A)));
        HIPCHK(top->d_vlossA.ensure((size_t)A));
        HIPCHK(hipMemcpyAsync(top->d_elatAA.p, elat.data(), sizeof(double) * (size_t)(A * A), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(top->d_elossAA.p, eloss.data(), sizeof(double) * (size_t)(A * A), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(top->d_vlossA.p, vl.data(), sizeof(double) * (size_t)A, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));  // the host vectors must outlive the async copies
        top->aaCols = top->attached;
        top->stats.pair_matrix_builds++;
    }
    // one launch: records, hops, row minima and the global minimum
    HIPCHK(hipEventRecord(top->ev0, st));
    HIPCHK(launch_pair_table_complete((int)A, c.row0, c.rows, top->d_elatAA.p, top->d_elossAA.p,
                                      top->d_vlossA.p, c.out_lr, c.out_hops, c.out_rowmin,
                                      top->d_stats.p, st));
    HIPCHK(hipEventRecord(top->ev1, st));
    return 0;
}

// The rows' sources and the target set (relabelled ids) to the device, not waited for; ev0 opens
// the kernels' event time.
int upload_endpoints(Topology* top, RowsCall& c) {
    const int64_t rows = c.rows, A = c.A;
    c.src.resize((size_t)rows);
    c.tgt.resize((size_t)A);
    for (int64_t i = 0; i < rows; i++) c.src[(size_t)i] = (uint32_t)top->hp->inv[(size_t)top->attached[(size_t)(c.row0 + i)]];
    for (int64_t i = 0; i < A; i++) c.tgt[(size_t)i] = (uint32_t)top->hp->inv[(size_t)top->attached[(size_t)i]];
    HIPCHK(top->d_sources.ensure((size_t)rows));
    HIPCHK(top->d_targets.ensure((size_t)A));
    HIPCHK(hipMemcpyAsync(top->d_sources.p, c.src.data(), sizeof(uint32_t) * (size_t)rows, hipMemcpyHostToDevice, c.st));
    HIPCHK(hipMemcpyAsync(top->d_targets.p, c.tgt.data(), sizeof(uint32_t) * (size_t)A, hipMemcpyHostToDevice, c.st));
    c.K = batch_k(top);
    top->stats.peeled_targets = 0;
    HIPCHK(hipEventRecord(top->ev0, c.st));
    return 0;
}

// The relaxation copy's target-derived content (bit 30 target marks, the records'
// target-aware kappa field, the rows re-sorted by it) belongs to one target set: a new
// set first restores the plain copy from d_adj (stale keys of an older set
// would cut rows that lead to the new targets), then prepares the new set if the
// target skip is on.  Blocks in the leaf-target records and the bit upload only;
// finish_target_prep reads the rest back.
int prepare_target_set(Topology* top, RowsCall& c) {
    hipStream_t st = c.st;
    const int64_t nadjk = (int64_t)(top->d_adjk.n / 4);
    // leaf targets: the records go with the launch, the copy's target-derived content
    // with the effective set -- a copy prepared the other way is restored first
    const bool leaf = leaf_targets_on(top);
    if (leaf) {
        CHK(ensure_leaf_targets(top, c.tgt, top->d_targets.p, st));
        c.ws.tleaf = top->d_tleaf.p;
    }
    top->stats.peeled_targets = leaf ? top->leafPeeled : 0;
    if (!top->adjkPlain && (top->adjkTargets != c.tgt || top->adjkLeaf != leaf)) {
        HIPCHK(launch_kappa_copy(top->g.V, nadjk, hub_segs(top), top->d_rowptr.p, adj_out(top), top->d_pot.p,
                                 top->d_sptPar.p, top->d_adjk.p, top->d_kap.p,
                                 top->d_ksum.p, top->d_kap0.p, st));
        top->adjkPlain = true;
        top->adjkFlagged = false;
        top->adjkResorted = false;
        top->adjkLeaf = false;
        top->adjkTargets.clear();
    }
    if (!top->targetSkip || !top->adjkPlain) return 0;
    // bit 30 of the relaxation copy's columns: the current target set.  Everything
    // after the bit upload is enqueued without a host sync: the GPU prepares the
    // target set while the host computes the source order (the fixpoint always
    // runs target_kappa iterations -- past its convergence an iteration reproduces its
    // input bit for bit -- and each iteration's change flag is read afterwards).
    CHK(upload_target_bits(top, c.tgt, st));
    HIPCHK(hipEventRecord(top->evp0, st));
    // (leaf targets: the effective set's bits, the peeled vertices dead)
    const uint32_t* tbits = leaf ? top->d_tbitsEff.p : top->d_tbits.p;
    const uint32_t* dead = leaf ? top->d_dead.p : nullptr;
    HIPCHK(launch_mark_targets(top->d_adjk.p, nadjk, tbits, st));
    // the records' kappa field: the target-aware fixpoint (kappa0 with 0 iterations)
    const int64_t V = top->g.V;
    const HubSegs hs = hub_segs(top);
    const int nit = std::max(0, top->targetKappa);
    HIPCHK(top->d_kfA.ensure(2 * (size_t)V));  // [K | Kt] (launch_kfix_step)
    HIPCHK(top->d_kfB.ensure(2 * (size_t)V));
    HIPCHK(top->d_kfPart.ensure(std::max<size_t>(1, hs.nseg)));
    HIPCHK(top->d_kfChanged.ensure((size_t)nit + 1));
    if (!top->kfKapReady) {  // the out-rows' static w - pi (once per graph)
        HIPCHK(top->d_kfKap.ensure((size_t)std::max<int64_t>(1, nadjk)));
        HIPCHK(launch_kfix_kap(adj_out(top), top->d_pot.p, nadjk, top->d_kfKap.p, st));
        top->kfKapReady = true;
    }
    HIPCHK(hipMemsetAsync(top->d_kfChanged.p, 0, sizeof(unsigned int) * ((size_t)nit + 1), st));
    HIPCHK(launch_kfix_step(top->d_rowptr.p, adj_out(top), top->d_kfKap.p, tbits,
                            nullptr, top->d_kfA.p, V, hs, top->d_kfPart.p,
                            top->d_kfChanged.p, st, dead));
    double* kin = top->d_kfA.p;
    double* kout = top->d_kfB.p;
    for (int it = 0; it < nit; it++) {
        HIPCHK(launch_kfix_step(top->d_rowptr.p, adj_out(top), top->d_kfKap.p,
                                tbits, kin, kout, V, hs, top->d_kfPart.p,
                                top->d_kfChanged.p + 1 + it, st, dead));
        std::swap(kin, kout);
    }
    if (top->targetResort) {
        KprimeScratch sc;
        CHK(ensure_kprime_scratch(top, &sc));
        HIPCHK(launch_kprime_resort(top->d_adjk.p, top->d_kap.p, top->d_ksum.p,
                                    top->d_kap0.p, top->d_rowptr.p, V, nadjk,
                                    top->d_pot.p, tbits, kin, sc, st));
    }
    HIPCHK(launch_kfix_store(top->d_adjk.p, nadjk, kin, st));
    top->kfFinal = kin;
    HIPCHK(hipEventRecord(top->evp1, st));
    top->tpPending = true;
    top->adjkTargets = c.tgt;
    top->adjkFlagged = true;
    top->adjkLeaf = leaf;
    top->adjkPlain = false;
    top->adjkResorted = top->targetResort;
    return 0;
}

// the asynchronous target preparation, after the build's closing event: iterations until the
// fixpoint and its event time (blocking copy)
int finish_target_prep(Topology* top) {
    if (!top->tpPending) return 0;
    top->tpPending = false;
    const int nit = std::max(0, top->targetKappa);
    std::vector<unsigned int> ch((size_t)nit + 1);
    HIPCHK(hipMemcpy(ch.data(), top->d_kfChanged.p, sizeof(unsigned int) * ch.size(),
                     hipMemcpyDeviceToHost));
    int it = 0;
    while (it < nit && ch[(size_t)it + 1]) it++;  // the first iteration that changed nothing
    top->stats.target_kappa_iters = it;
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, top->evp0, top->evp1));
    top->stats.target_prep_ms = ms;  // its GPU time (overlapped with the source order)
    return 0;
}

// Tie probe (integer latencies, before the first batched build of the topology):
// the batch kernel on kTieProbeRows sample rows (the range's first rows, written in
// place); if >= 90 % of them cross a d-tied parent the topology is tie-dense and
// every row goes straight to the heap replay -- the batch kernel would only compute
// rows the replay recomputes (C4-int: 0.93 s of batch kernel per first build).
// One launch; the host waits for its row flags, and again after the counters start over.
int tie_probe(Topology* top, RowsCall& c) {
    if (!top->tieReplay || top->tieDenseOpt >= 0 || top->tieDense || top->tieProbed ||
        c.rows < 2 * kTieProbeRows)
        return 0;
    edge_scan(top);
    if (!top->replayIntOk) return 0;
    hipStream_t st = c.st;
    top->tieProbed = true;
    const auto tq0 = std::chrono::steady_clock::now();
    const int64_t P = kTieProbeRows;
    const double delta = default_delta(top);
    const std::vector<double> sh = source_shifts(top, c.src.data(), P, delta);
    HIPCHK(top->d_probeSrc.ensure((size_t)P));
    HIPCHK(top->d_probeSh.ensure((size_t)P));
    HIPCHK(hipMemcpyAsync(top->d_probeSrc.p, c.src.data(), 4 * (size_t)P, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(top->d_probeSh.p, sh.data(), 8 * (size_t)P, hipMemcpyHostToDevice, st));
    const std::vector<double> hs = source_h0_seeds(top, c.src.data(), P);
    HIPCHK(top->d_probeSeed.ensure((size_t)P));
    HIPCHK(hipMemcpyAsync(top->d_probeSeed.p, hs.data(), 8 * (size_t)P, hipMemcpyHostToDevice, st));
    SlotWs pws = c.ws;
    pws.rowmap = nullptr;  // sample row i -> output row i
    const SsspLdsPlan bp = batch_lds_plan(top, c.K);
    CHK(hub_rows_ready(top, bp.H, st));
    HIPCHK(launch_sssp_batch(c.K, dev_csr(top), pws, top->d_probeSrc.p, top->d_probeSh.p,
                             top->d_probeSeed.p, (int)P, c.K, top->d_targets.p, (int)c.A, delta, bp,
                             top->iterGuard, c.out_lr, c.out_hops, c.out_rowmin,
                             top->d_stats.p, st));
    std::vector<uint8_t> fl((size_t)P);
    HIPCHK(hipMemcpyAsync(fl.data(), top->d_rowflag.p, (size_t)P, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t nf = 0;
    for (uint8_t x : fl) nf += x ? 1 : 0;
    top->stats.tie_probe_rows = P;
    top->stats.tie_probe_flagged = nf;
    if (nf * 10 >= P * 9) top->tieDense = true;
    // the build's statistics and row flags start over (the rows are recomputed)
    CHK(reset_dev_stats(top, st));
    HIPCHK(hipMemsetAsync(top->d_rowflag.p, 0, (size_t)c.rows, st));
    HIPCHK(hipStreamSynchronize(st));
    top->stats.tie_probe_ms = std::chrono::duration<double, std::milli>(
        std::chrono::steady_clock::now() - tq0).count();
    return 0;
}

// sources per batch: a shard that leaves slots idle at K (8-GPU builds: 1250
// rows = 157 batches for 256 slots) spreads over every slot with fewer sources
// per batch (C4, 1250 rows: 89.7 -> 83.2 ms).  With more than one round it does
// not pay (2500 rows at 5 per batch: 146 -> 158 ms).
int batch_fill_for(int64_t rows, int K, int slots, int option) {
    if (option > 0) return std::min(K, option);
    // the fewest sources per batch that still finish the rows in the fewest
    // rounds of the slots: a batch's time grows with its sources, so equal
    // rounds of smaller batches beat a last round of a few full ones (2,500
    // rows on 256 slots: 500 batches of 5, two even rounds, instead of 313
    // batches of 8 whose last 57 form a second round on their own)
    const int64_t S = std::max(1, slots);
    const int64_t rounds = (rows + (int64_t)K * S - 1) / ((int64_t)K * S);
    return (int)std::max<int64_t>(1, std::min<int64_t>(K, (rows + rounds * S - 1) / (rounds * S)));
}

// Batches of K sources settle in lock-step and share an expansion when their
// shifted distances to a vertex fall in one bucket: sources whose shortest paths
// enter the hub core through the same hub share the most.  Batch position p takes
// source perm[p]; the kernel writes its row at rowmap[p] = perm[p].
// The grouping order of the sources src (option source_order) on a V-vertex graph.
std::vector<uint32_t> group_sources(int sourceOrder, const std::vector<uint32_t>& src,
                                    const HostPrep& hp, int64_t V) {
    const int64_t rows = (int64_t)src.size();
    std::vector<uint32_t> perm((size_t)rows);
    std::iota(perm.begin(), perm.end(), 0u);
    if (sourceOrder == 2) {
        // preorder of the h0 shortest-path tree (children by ascending vertex id):
        // sources in one subtree (sharing the longest path prefix from h0) are
        // adjacent.  Preorder = lexicographic order of the root-first parent paths;
        // the forest's preorder (HostPrep::preorder, from the graph preparation)
        // numbers h0's tree first, then the other roots' trees
        const std::vector<uint32_t>& pre = hp.preorder;
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
            return pre[src[a]] < pre[src[b]];
        });
    } else if (sourceOrder == 1) {
        const uint32_t Hc = (uint32_t)std::min<int64_t>(kGroupHubs, V);
        std::vector<uint64_t> key((size_t)rows);
        for (int64_t i = 0; i < rows; i++) {
            uint32_t v = src[(size_t)i];
            for (int hop = 0; v >= Hc && hop < 64; hop++) {  // up the h0 tree
                const uint32_t p = hp.sptPar[(size_t)v];
                if (p == 0xFFFFFFFFu) break;
                v = p;
            }
            const double pi = hp.pot[(size_t)src[(size_t)i]];
            const float pf = std::isfinite(pi) ? (float)pi : INFINITY;
            uint32_t pb;
            memcpy(&pb, &pf, 4);
            key[(size_t)i] = ((uint64_t)v << 32) | pb;  // pi >= 0: bits order as values
        }
        std::stable_sort(perm.begin(), perm.end(),
                         [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    }
    return perm;
}

// order of the batches (groups of kf consecutive positions of perm) in the dequeue: the
// kernel ends with the slowest slot, so the last batches decide its tail
// batch_order 5 (auto, resolved by the caller): by depth when the batches fill more than 3
// rounds of the slots -- longest-predicted first shortens the tail of a many-round launch (full
// table: 71.1 -> 68.5 ms) -- else by pi: with two rounds the order only pairs
// batches, and the depth predictor pairs them worse (2,500 rows: 25.9 -> 28.6 ms)
std::vector<uint32_t> order_batches(int border, int kf, const std::vector<uint32_t>& src,
                                    const HostPrep& hp, std::vector<uint32_t> perm) {
    const int64_t rows = (int64_t)perm.size();
    if (border == 0 || rows <= kf) return perm;
    const int64_t nb = (rows + kf - 1) / kf;
    std::vector<uint32_t> bo((size_t)nb);
    std::iota(bo.begin(), bo.end(), 0u);
    if (border == 1) {
        SplitMix rng(0x5eedull);
        for (int64_t i = nb - 1; i > 0; i--) std::swap(bo[(size_t)i], bo[(size_t)rng.below((uint64_t)i + 1)]);
    } else {
        std::vector<double> mp((size_t)nb, 0.0);
        for (int64_t i = 0; i < rows; i++) {
            const uint32_t s = src[(size_t)perm[(size_t)i]];
            if (border == 4) {
                // the source's depth in the h0 shortest-path tree: deeper
                // sources relax more pairs (C4: corr 0.59 with the batch's
                // duration, against 0.25 for mean pi)
                mp[(size_t)(i / kf)] += (double)hp.depth[s];
            } else {
                const double p = hp.pot[(size_t)s];
                mp[(size_t)(i / kf)] += std::isfinite(p) ? p : 0.0;
            }
        }
        for (int64_t b = 0; b < nb; b++) mp[(size_t)b] /= (double)(std::min(rows, (b + 1) * kf) - b * kf);
        const bool desc = border != 3;
        std::stable_sort(bo.begin(), bo.end(), [&](uint32_t a, uint32_t b) {
            return desc ? mp[a] > mp[b] : mp[a] < mp[b];
        });
    }
    // the ragged batch (if any) stays last
    const int64_t last = nb - 1;
    if (rows % kf) {
        auto it = std::find(bo.begin(), bo.end(), (uint32_t)last);
        bo.erase(it);
        bo.push_back((uint32_t)last);
    }
    std::vector<uint32_t> p2;
    p2.reserve((size_t)rows);
    for (uint32_t b : bo)
        for (int64_t i = (int64_t)b * kf; i < std::min(rows, ((int64_t)b + 1) * kf); i++)
            p2.push_back(perm[(size_t)i]);
    return p2;
}

// the order, the row map and the bucket shifts depend only on the sources, the
// batch fill and the options: a rebuild of the same rows reuses them (the ord* cache)
void cached_order(Topology* top, const RowsCall& c) {
    const int64_t nbat = (c.rows + c.kf - 1) / c.kf;
    const int border = top->batchOrder != 5 ? top->batchOrder
                       : nbat > 3 * (int64_t)std::max(1, c.ws.slots) ? 4 : 2;
    const bool cached = top->ordHp == top->hp.get() && top->ordKf == c.kf &&
                        top->ordSO == top->sourceOrder && top->ordBO == border &&
                        top->ordDelta == c.delta && top->ordPhase == h0_phase(top, c.delta) &&
                        top->ordSrc == c.src;
    if (cached) return;
    std::vector<uint32_t> perm = group_sources(top->sourceOrder, c.src, *top->hp, top->g.V);
    top->ordBase = perm;  // the grouping order (the measured layout starts from it)
    top->ordPerm = order_batches(border, c.kf, c.src, *top->hp, std::move(perm));
    top->ordSrc = c.src;
    top->ordHp = top->hp.get();
    top->ordKf = c.kf;
    top->ordSO = top->sourceOrder;
    top->ordBO = border;
    top->ordDelta = c.delta;
    top->ordPhase = h0_phase(top, c.delta);
    top->ordUploaded = false;
}

// The batched launch: the layout's upload (blocking; a cached order that is already there is
// not sent again), which closes order_ms (started at to0); then ev0, the hub rows' refill, the
// launch and ev1, and the host waits for the kernel (build steps 2 and 3).
int launch_batches(Topology* top, RowsCall& c, std::chrono::steady_clock::time_point to0) {
    const int64_t rows = c.rows;
    const int kf = c.kf;
    hipStream_t st = c.st;
    SlotWs& ws = c.ws;
    // the launch's layout: batches sized and ordered by the sources' measured costs
    // (option balance, once every source has one), else the cached order
    std::vector<uint32_t> lperm, lstart;
    const bool measured =
        top->balance && measured_layout(top, c.src, kf, ws.slots, lperm, lstart);
    if (measured || !top->ordUploaded) {
        const std::vector<uint32_t>& perm = measured ? lperm : top->ordPerm;
        CHK(upload_layout(top, c.src, perm, measured ? &lstart : nullptr, c.delta, st));
        top->ordUploaded = !measured;
    }
    if (!measured) {
        const int64_t nbat = (rows + kf - 1) / kf;
        lstart.resize((size_t)nbat + 1);
        for (int64_t b = 0; b <= nbat; b++) lstart[(size_t)b] = (uint32_t)std::min(rows, b * kf);
    }
    ws.bstart = measured ? top->d_bstart.p : nullptr;
    ws.nbat = measured ? (int)(lstart.size() - 1) : 0;
    const int64_t lnbat = (int64_t)lstart.size() - 1;
    top->slotsUsed = (int)std::min<int64_t>(ws.slots, lnbat);
    top->stats.batch_layout_measured = measured ? 1 : 0;
    top->lastBatches = lnbat;
    ws.rowmap = top->d_rowmap.p;
    // per batch {start tick, end tick, slot, near iterations, sweeps, expansions,
    // relaxations, sources, ...} (kBTraceWords u64): the batch times give the sources'
    // costs (option balance); SHD_BATCH_TRACE=<file> (diagnostic) appends them, then
    // per batch position {source vertex, pi bits}
    const char* btf = getenv("SHD_BATCH_TRACE");
    if (top->balance || (btf && *btf)) {
        HIPCHK(top->d_btrace.ensure((size_t)lnbat * kBTraceWords));
        ws.btrace = top->d_btrace.p;
    }
    top->stats.order_ms = std::chrono::duration<double, std::milli>(
        std::chrono::steady_clock::now() - to0).count();
    HIPCHK(hipEventRecord(top->ev0, st));
    const SsspLdsPlan bp = batch_lds_plan(top, c.K);
    top->stats.lds_hubs = bp.H;
    CHK(hub_rows_ready(top, bp.H, st));
    bstep_mark(top, 2);
    HIPCHK(launch_sssp_batch(c.K, dev_csr(top), ws, top->d_bsrc.p,
                             top->d_srcsh.p, top->d_h0seed.p, (int)rows,
                             measured ? c.K : kf, top->d_targets.p,
                             (int)c.A, c.delta, bp, top->iterGuard, c.out_lr, c.out_hops,
                             c.out_rowmin, top->d_stats.p, st));
    CHK(close_and_wait(top, st));  // the kernel's wall time goes to step 3
    bstep_mark(top, 3);
    if (ws.btrace) {  // read back after the build's closing event (read_batch_trace)
        c.bt.kf = measured ? 0 : kf;
        c.bt.slots = ws.slots;
        c.bt.start.swap(lstart);
        c.bt.file = btf;
    }
    return 0;
}

// The batch kernel's part of a build: workspace and row flags, the target set's preparation
// (asynchronous), the tie probe, then -- unless it found the topology tie-dense -- the batch
// fill, the source and batch order (order_ms: host work that overlaps the preparation) and the
// launch.
int enqueue_batched(Topology* top, RowsCall& c) {
    CHK(ensure_workspace(top, (int)c.rows));
    HIPCHK(top->d_rowflag.ensure((size_t)c.rows));
    HIPCHK(hipMemsetAsync(top->d_rowflag.p, 0, (size_t)c.rows, c.st));
    c.ws = slot_ws(top);
    c.ws.rowflag = top->d_rowflag.p;
    CHK(prepare_target_set(top, c));
    CHK(tie_probe(top, c));
    c.probeDense = top->tieReplay && top->tieDenseOpt < 0 && top->tieDense;
    if (c.probeDense) return 0;
    const auto to0 = std::chrono::steady_clock::now();
    c.kf = batch_fill_for(c.rows, c.K, c.ws.slots, top->batchFill);
    top->stats.batch_fill = c.kf;
    // workgroups the launch uses: the batches, at most the workspace's slots (it
    // may hold more: sized for a full table by the attach-time preparation)
    top->slotsUsed = (int)std::min<int64_t>(c.ws.slots, (c.rows + c.kf - 1) / c.kf);
    c.delta = default_delta(top);
    cached_order(top, c);
    return launch_batches(top, c, to0);
}

// the batch times: the sources' costs (option balance) and the SHD_BATCH_TRACE file -- after
// ev1, so the copy (blocking) and the host work stay out of the kernel's event time
int read_batch_trace(Topology* top, const RowsCall& c) {
    if (c.bt.start.empty()) return 0;
    const int64_t lnbat = (int64_t)c.bt.start.size() - 1;
    const std::vector<uint32_t>& psrc = top->layPsrc;
    std::vector<unsigned long long> bv((size_t)lnbat * kBTraceWords);
    HIPCHK(hipMemcpy(bv.data(), top->d_btrace.p, 8 * kBTraceWords * (size_t)lnbat, hipMemcpyDeviceToHost));
    if (top->balance) record_costs(top, psrc, c.bt.start, bv);
    FILE* f = c.bt.file && *c.bt.file ? fopen(c.bt.file, "ab") : nullptr;
    if (!f) return 0;
    const int64_t hdr[4] = {lnbat, (int64_t)c.bt.kf, (int64_t)c.bt.slots, c.rows};
    fwrite(hdr, 8, 4, f);
    fwrite(bv.data(), 8, bv.size(), f);
    for (int64_t i = 0; i < c.rows; i++) {
        const double p = top->hp->pot[(size_t)psrc[(size_t)i]];
        const int64_t rec[2] = {(int64_t)psrc[(size_t)i], 0};
        fwrite(rec, 8, 1, f);
        fwrite(&p, 8, 1, f);
    }
    fclose(f);
    return 0;
}

// rows that need igraph's heap pop order: replayed exactly on the GPU.  The row
// flags come back with a blocking copy; the replay's uploads block, its launch sits between evr0
// and evr1 and the host waits for it.
int replay_rows(Topology* top, RowsCall& c) {
    const int64_t rows = c.rows;
    hipStream_t st = c.st;
    std::vector<uint32_t> rlist;
    top->stats.tie_dense = c.dense || c.probeDense ? 1 : 0;
    if (c.allReplay || c.probeDense) {
        rlist.resize((size_t)rows);
        std::iota(rlist.begin(), rlist.end(), 0u);
    } else if (top->tieReplay) {
        std::vector<uint8_t> fl((size_t)rows);
        HIPCHK(hipMemcpy(fl.data(), top->d_rowflag.p, (size_t)rows, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < rows; i++)
            if (fl[(size_t)i]) rlist.push_back((uint32_t)i);
        if (rows >= 64 && (int64_t)rlist.size() * 10 >= rows * 9) top->tieDense = true;
    }
    top->replayPending = false;
    // builds that run only the replay (tie-dense, directed, multigraph, replay_all): the
    // batch workspace (~110 GB at C4) goes back so the replay can hold more rows at once
    if (c.allReplay || c.probeDense) release_workspace(top);
    if (rlist.empty()) return 0;
    CHK(upload_replay(top));
    CHK(ensure_replay_ws(top, (int)rlist.size()));
    CHK(upload_target_bits(top, c.tgt, st));
    HIPCHK(top->d_rrows.ensure(rlist.size()));
    HIPCHK(hipMemcpy(top->d_rrows.p, rlist.data(), 4 * rlist.size(), hipMemcpyHostToDevice));
    HIPCHK(hipEventRecord(top->evr0, st));
    HIPCHK(launch_heap_replay(replay_csr(top), replay_ws(top), top->d_sources.p,
                              top->d_rrows.p, (int)rlist.size(), top->d_targets.p, (int)c.A,
                              0, c.out_lr, c.out_hops, c.out_rowmin, top->d_stats.p, nullptr,
                              nullptr, st));
    HIPCHK(hipEventRecord(top->evr1, st));
    HIPCHK(hipStreamSynchronize(st));
    top->replayPending = true;
    return 0;
}

}  // namespace

// Enqueue rows [row0,row1) into out buffers (device pointers) on `st`.
int enqueue_rows(Topology* top, int64_t row0, int64_t row1, double2* out_lr, uint16_t* out_hops,
                 double* out_rowmin, hipStream_t st) {
    RowsCall c;
    c.row0 = row0;
    c.rows = row1 - row0;
    c.A = top->A;
    c.out_lr = out_lr;
    c.out_hops = out_hops;
    c.out_rowmin = out_rowmin;
    c.st = st;
    if (c.rows <= 0 || c.A <= 0) return 0;
    CHK(reset_dev_stats(top, st));
    if (top->isComplete) {
        CHK(enqueue_complete(top, c));
    } else {
        CHK(upload_csr(top));
        // the "replay_all" test hook runs every row through the exact heap replay; otherwise
        // the batch kernel runs (directed topologies too: out-rows relaxed, parents from the
        // in-rows) and flags the rows that need it
        // multigraphs too: the reference sums the igraph_get_eid edge of each hop, which the batch
        // epilogue (latency = distance) does not reproduce when parallel edges differ
        c.dense = top->tieReplay && (top->tieDenseOpt == 1 ||
                                     (top->tieDenseOpt < 0 && top->tieDense));
        c.allReplay = top->replayAll || top->hasMultiEdges || c.dense;
        CHK(upload_endpoints(top, c));
        if (!c.allReplay) CHK(enqueue_batched(top, c));
        CHK(close_and_wait(top, st));
        CHK(finish_target_prep(top));
        CHK(read_batch_trace(top, c));
        CHK(replay_rows(top, c));
    }
    top->rowsPending = true;
    top->stats.batch = top->isComplete ? 0 : batch_k(top);
    top->stats.sources = c.rows;
    top->stats.targets = c.A;
    return 0;
}

int collect_row_stats(Topology* top) {
    if (!top->rowsPending) return 0;
    HIPCHK(hipEventSynchronize(top->ev1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, top->ev0, top->ev1));
    unsigned long long h[ST_COUNT];
    HIPCHK(hipMemcpy(h, top->d_stats.p, sizeof h, hipMemcpyDeviceToHost));
    top->stats.sssp_kernel_ms = ms;
    top->stats.build_ms = ms;
    top->stats.replay_ms = 0.0;
    if (top->replayPending) {
        float rms = 0;
        HIPCHK(hipEventSynchronize(top->evr1));
        HIPCHK(hipEventElapsedTime(&rms, top->evr0, top->evr1));
        top->stats.replay_ms = rms;
        top->stats.build_ms += rms;
        top->replayPending = false;
    }
    ShdStats& s = top->stats;
    int khz = 0;  // the kernels' tick counters are wall-clock ticks
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, top->devId) != hipSuccess || khz <= 0)
        khz = 100000;
    // the whole build
    s.errors = (int64_t)h[ST_ERRORS];
    s.slots = top->isComplete ? 0 : (top->slotsUsed > 0 ? top->slotsUsed : top->slots);
    s.batches = top->lastBatches;
    double gm;
    memcpy(&gm, &h[ST_GLOBAL_MIN], sizeof gm);
    top->eagerMin = std::isinf(gm) ? -1.0 : gm;
    // batch kernel
    s.relaxations = (int64_t)h[ST_RELAX];
    s.near_iterations = (int64_t)h[ST_NEAR_IT];
    s.far_splits = (int64_t)h[ST_SPLITS];
    s.far_scan_sources = (int64_t)h[ST_FARSCAN];
    s.touched_lines = (int64_t)h[ST_TOUCHED];
    for (int i = 0; i < 4; i++) s.phase_ms[i] = (double)h[ST_T_INIT + i] / (double)khz;
    s.split_ms = (double)h[ST_T_SPLIT] / (double)khz;
    for (int i = 0; i < 8; i++) s.events[i] = (int64_t)h[ST_EV0 + i];
    if (h[ST_OVERSITE]) WARNING("queue overflow sites 0x%llx", h[ST_OVERSITE]);
    if (h[ST_FARSCAN])
        MESSAGE("%llu sources overflowed the far pile and finished with scanning splits",
                h[ST_FARSCAN]);
    // parent pass and path walk
    s.ambiguous_pairs = (int64_t)h[ST_AMBIGUOUS];
    s.long_paths = (int64_t)h[ST_LONGPATH];
    s.walk_steps = (int64_t)h[ST_WALK];
    for (int i = 0; i < 4; i++) s.walk_kinds[i] = (int64_t)h[ST_WK0 + i];
    for (int i = 0; i < 4; i++) s.parent_phase_ms[i] = (double)h[ST_PT0 + i] / (double)khz;
    // heap replay
    s.replay_rows = (int64_t)h[ST_RP_ROWS];
    s.replay_pops = (int64_t)h[ST_RP_POPS];
    s.replay_pushes = (int64_t)h[ST_RP_PUSH];
    s.replay_modifies = (int64_t)h[ST_RP_MOD];
    s.replay_skips = (int64_t)h[ST_RP_SKIP];
    s.replay_slots = s.replay_rows ? std::min(top->rslots, top->rslotsUse) : 0;
    s.replay_int_keys = s.replay_rows && top->replayIntOpt && top->replayIntOk ? 1 : 0;
    // profiling builds (SHD_RP_LINES, SHD_RP_TIME, SHD_BATCH_TIME, SHD_BATCH_WRCOUNT)
    for (int i = 0; i < 6; i++) s.replay_lines[i] = (int64_t)h[ST_RP_L0 + i];
    for (int i = 0; i < 4; i++) s.replay_phase_ms[i] = (double)h[ST_RP_T0 + i] / (double)khz;
    s.replay_sink_rounds = (int64_t)h[ST_RP_T0 + 4];
    s.replay_heap_sum = (int64_t)h[ST_RP_T0 + 5];
    for (int i = 0; i < 3; i++) s.replay_sink_ms[i] = (double)h[ST_RP_T0 + 6 + i] / (double)khz;
    s.replay_pf_hits = (int64_t)h[ST_RP_T0 + 9];
    for (int i = 0; i < 6; i++) s.batch_wave_ms[i] = (double)h[ST_BT0 + i] / (double)khz;
    s.batch_rounds = (int64_t)h[ST_BT0 + 6];
    s.batch_edges_b = (int64_t)h[ST_BT0 + 7];
    for (int i = 0; i < 4; i++) s.sweep_events[i] = (int64_t)h[ST_SW0 + i];
    for (int i = 0; i < 16; i++) s.write_lines[i] = (int64_t)h[ST_WL0 + i];
    for (int i = 0; i < 8; i++) s.read_lines[i] = (int64_t)h[ST_RL0 + i];
    if (h[ST_OVERFLOW]) CRITICAL("SSSP queue overflow / iteration guard (code %llu)", h[ST_OVERFLOW]);
    if (s.ambiguous_pairs && !top->tieReplay)
        WARNING("%lld pairs cross a parent tie (equal d[u]): igraph's heap pop order decides them "
                "in the reference; tie_replay is off, so the lowest adjacency slot is used here",
                (long long)s.ambiguous_pairs);
    top->rowsPending = false;
    return h[ST_OVERFLOW] ? -4 : 0;
}

// ---------------------------------------------------------------------------------------------
// multi-GPU build inside one process: no Python, no torch.distributed
// ---------------------------------------------------------------------------------------------
// RCCL is loaded on first use (dlopen by soname: a process that already holds RCCL, e.g. through
// torch, shares that copy; a single-GPU user never needs it).
struct RcclApi {
    bool ok = false;
    std::string why;
    ncclResult_t (*commInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*commDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*allGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*allReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                              hipStream_t) = nullptr;
    ncclResult_t (*groupStart)() = nullptr;
    ncclResult_t (*groupEnd)() = nullptr;
    const char* (*errStr)(ncclResult_t) = nullptr;
};

RcclApi& rccl() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = nullptr;
        for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) {
            api.why = dlerror() ? dlerror() : "librccl.so.1 not found";
            return;
        }
        auto sym = [&](const char* n) { return dlsym(h, n); };
        api.commInitAll = (decltype(api.commInitAll))sym("ncclCommInitAll");
        api.commDestroy = (decltype(api.commDestroy))sym("ncclCommDestroy");
        api.allGather = (decltype(api.allGather))sym("ncclAllGather");
        api.allReduce = (decltype(api.allReduce))sym("ncclAllReduce");
        api.groupStart = (decltype(api.groupStart))sym("ncclGroupStart");
        api.groupEnd = (decltype(api.groupEnd))sym("ncclGroupEnd");
        api.errStr = (decltype(api.errStr))sym("ncclGetErrorString");
        api.ok = api.commInitAll && api.commDestroy && api.allGather && api.allReduce &&
                 api.groupStart && api.groupEnd && api.errStr;
        if (!api.ok) api.why = "RCCL symbols missing";
    });
    return api;
}

#define NCCLCHK(expr)                                                                        \
    do {                                                                                     \
        ncclResult_t _r = (expr);                                                            \
        if (_r != ncclSuccess) {                                                             \
            CRITICAL("RCCL error %s at %s:%d (%s)", rccl().errStr(_r), __FILE__, __LINE__, #expr); \
            return -200 - (int)_r;                                                           \
        }                                                                                    \
    } while (0)

int num_devices() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

Topology* make_peer(Topology* top, int phys) {
    Topology* p = new Topology(top->gp);
    p->isComplete = top->isComplete;
    p->isDirected = top->isDirected;
    p->hasMultiEdges = top->hasMultiEdges;
    p->abortOnError = top->abortOnError.load();
    p->lazy = false;
    p->device = phys;
    p->isPeer = true;
    return p;
}

// options and columns of the owner, copied before every multi-device build
void sync_peer(Topology* top, Topology* p) {
    p->delta = top->delta;
    p->slotsOpt = top->slotsOpt;
    p->hubLimit = top->hubLimit;
    p->parHubs = top->parHubs;
    p->rsChunk = top->rsChunk;
    p->batchK = top->batchK;
    p->iterGuard = top->iterGuard;
    p->tieReplay = top->tieReplay;
    p->replayAll = top->replayAll;
    p->tieDenseOpt = top->tieDenseOpt;
    p->tieDense = p->tieDense || top->tieDense;
    p->replaySlotsOpt = top->replaySlotsOpt;
    p->replayLandmark = top->replayLandmark;
    p->replayIntOpt = top->replayIntOpt;
    if (top->meanLat >= 0 && !(p->meanLat >= 0)) {  // the owner's edge scan (same graph)
        p->minLat = top->minLat;
        p->meanLat = top->meanLat;
        p->replayIntOk = top->replayIntOk;
    }
    p->sourceOrder = top->sourceOrder;
    p->balance = top->balance;
    p->batchOrder = top->batchOrder;
    p->batchFill = top->batchFill;
    p->h0Phase = top->h0Phase;
    p->h0PhaseSet = top->h0PhaseSet;
    p->targetSkip = top->targetSkip;
    p->targetKappa = top->targetKappa;
    p->targetResort = top->targetResort;
    p->leafTargets = top->leafTargets;
    if (p->h0Seed != top->h0Seed) {
        p->h0Seed = top->h0Seed;
        p->ordUploaded = false;
    }
    p->attached = top->attached;
    p->colOf = top->colOf;
    p->A = top->A;
    p->geomInit = true;
}

template <class T>
hipError_t peer_copy(DevBuf<T>& dst, int ddev, const DevBuf<T>& src, int sdev, hipStream_t st) {
    if (!src.p || src.n == 0) return hipSuccess;
    const hipError_t e = dst.ensure(src.n);
    if (e != hipSuccess) return e;
    return hipMemcpyPeerAsync(dst.p, ddev, src.p, sdev, sizeof(T) * src.n, st);
}

// A peer engine takes the owner's prepared graph: the device CSR and landmark arrays are copied
// device to device (xGMI peer copies; the same device for a test configuration) and the host side
// is shared -- the graph is prepared once per multi-GPU build, not once per device.
int copy_csr_from(Topology* p, int pdev, Topology* o, int odev) {
    hipStream_t st = p->stream;
    if (pdev != odev) {
        const hipError_t e = hipDeviceEnablePeerAccess(odev, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
            (void)hipGetLastError();  // no direct access: the copies are staged by the runtime
    }
    HIPCHK(peer_copy(p->d_rowptr, pdev, o->d_rowptr, odev, st));
    HIPCHK(peer_copy(p->d_adj, pdev, o->d_adj, odev, st));
    HIPCHK(peer_copy(p->d_adjo, pdev, o->d_adjo, odev, st));
    HIPCHK(peer_copy(p->d_rowptrIn, pdev, o->d_rowptrIn, odev, st));
    HIPCHK(peer_copy(p->d_adjk, pdev, o->d_adjk, odev, st));
    HIPCHK(peer_copy(p->d_kap, pdev, o->d_kap, odev, st));
    HIPCHK(peer_copy(p->d_ksum, pdev, o->d_ksum, odev, st));
    HIPCHK(peer_copy(p->d_kap0, pdev, o->d_kap0, odev, st));
    HIPCHK(peer_copy(p->d_spt, pdev, o->d_spt, odev, st));
    HIPCHK(peer_copy(p->d_sptPar, pdev, o->d_sptPar, odev, st));
    HIPCHK(peer_copy(p->d_pot, pdev, o->d_pot, odev, st));
    HIPCHK(peer_copy(p->d_aloss, pdev, o->d_aloss, odev, st));
    HIPCHK(peer_copy(p->d_vloss, pdev, o->d_vloss, odev, st));
    HIPCHK(peer_copy(p->d_selfLat, pdev, o->d_selfLat, odev, st));
    HIPCHK(peer_copy(p->d_selfLoss, pdev, o->d_selfLoss, odev, st));
    HIPCHK(peer_copy(p->d_eu, pdev, o->d_eu, odev, st));
    HIPCHK(peer_copy(p->d_ev, pdev, o->d_ev, odev, st));
    HIPCHK(peer_copy(p->d_elat, pdev, o->d_elat, odev, st));
    HIPCHK(peer_copy(p->d_eloss, pdev, o->d_eloss, odev, st));
    HIPCHK(peer_copy(p->d_inv, pdev, o->d_inv, odev, st));
    HIPCHK(peer_copy(p->d_hseg, pdev, o->d_hseg, odev, st));
    HIPCHK(peer_copy(p->d_hmulti, pdev, o->d_hmulti, odev, st));
    p->hsegRows = o->hsegRows;
    p->hsegN = o->hsegN;
    p->hmultiN = o->hmultiN;
    HIPCHK(hipStreamSynchronize(st));
    p->hp = o->hp;
    p->rowsSorted = o->rowsSorted;
    p->adjkPlain = o->adjkPlain;
    p->adjkFlagged = o->adjkFlagged;
    p->adjkResorted = o->adjkResorted;
    p->adjkLeaf = o->adjkLeaf;
    p->adjkTargets = o->adjkTargets;
    p->csrUploaded = true;
    return 0;
}

void release_comms(Topology* top) {
    if (!top->comms.empty() && rccl().ok)
        for (ncclComm_t c : top->comms) (void)rccl().commDestroy(c);
    top->comms.clear();
}

namespace {
using clk = std::chrono::steady_clock;

// what the threads and the exchange of one build_multi call share
struct MultiBuild {
    Topology* top = nullptr;
    int N = 1;
    int64_t A = 0, R = 0;     // columns; rows per shard
    std::vector<int> phys;    // the slots' physical devices
    bool push = false;        // the shards push their rows (else RCCL once all are done)
    std::vector<uint8_t> pdid;             // per slot: the peer preparation copied the graph
    std::vector<unsigned long long> dmin;  // ... its rows' minimum (f64 bits)
    std::vector<int64_t> drows;            // ... its rows
    std::vector<clk::time_point> tdone, tpushed;  // ... when they were built, and pushed
};

// thread of peer d before the build: its device (a device's first stream costs ~80 ms of HIP
// queue setup), the owner's edge scan and, first time, the owner's prepared graph
int prepare_peer(int d, MultiBuild& m) {
    Topology* top = m.top;
    Topology* T = slot_engine(top, d);
    reset_build_stats(T);
    HIPCHK(hipSetDevice(m.phys[(size_t)d]));
    CHK(dev_init(T));
    T->minLat = top->minLat;
    T->meanLat = top->meanLat;
    T->replayIntOk = top->replayIntOk;  // the owner's edge scan (same graph)
    if (!top->isComplete && !T->csrUploaded) {
        CHK(copy_csr_from(T, m.phys[(size_t)d], top, m.phys[0]));
        m.pdid[(size_t)d] = 1;
    }
    return 0;
}

// thread of slot d: rows [d R, (d+1) R) on its device, then (push) the rows into every other
// device's table on its exchange stream, waited for
int build_shard(int d, MultiBuild& m) {
    Topology* top = m.top;
    Topology* T = slot_engine(top, d);
    const int N = m.N;
    const int64_t A = m.A, R = m.R;
    const std::vector<int>& phys = m.phys;
    HIPCHK(hipSetDevice(phys[(size_t)d]));
    CHK(dev_init(T));
    HIPCHK(hipSetDevice(phys[(size_t)d]));
    const int64_t r0 = std::min(A, d * R), r1 = std::min(A, r0 + R);
    if (r1 > r0) {
        CHK(enqueue_rows(T, r0, r1, T->d_lr.p + r0 * A, T->d_hops.p + r0 * A,
                         T->d_rowmin.p + r0, T->stream));
        CHK(collect_row_stats(T));
        HIPCHK(hipMemcpy(&m.dmin[(size_t)d], T->d_stats.p + ST_GLOBAL_MIN, 8, hipMemcpyDeviceToHost));
    }
    m.drows[(size_t)d] = r1 - r0;
    m.tdone[(size_t)d] = clk::now();
    if (m.push && r1 > r0) {  // this shard into every other device's table, now
        for (int e = 0; e < N; e++) {
            if (e == d) continue;
            Topology* S = slot_engine(top, e);
            const int pd = phys[(size_t)e], ps = phys[(size_t)d];
            const size_t n = (size_t)((r1 - r0) * A);
            HIPCHK(hipMemcpyPeerAsync(S->d_lr.p + r0 * A, pd, T->d_lr.p + r0 * A, ps, sizeof(double2) * n, T->xstream));
            HIPCHK(hipMemcpyPeerAsync(S->d_hops.p + r0 * A, pd, T->d_hops.p + r0 * A, ps, 2 * n, T->xstream));
            HIPCHK(hipMemcpyPeerAsync(S->d_rowmin.p + r0, pd, T->d_rowmin.p + r0, ps, 8 * (size_t)(r1 - r0), T->xstream));
        }
        HIPCHK(hipStreamSynchronize(T->xstream));
    }
    m.tpushed[(size_t)d] = clk::now();
    return 0;
}

// RCCL exchange: all-gathers of the rows, hops and row minima in place, an all-reduce of the
// devices' minima; every engine's stream waited for
int exchange_rccl(MultiBuild& m) {
    Topology* top = m.top;
    const int N = m.N;
    const int64_t A = m.A, R = m.R;
    RcclApi& api = rccl();
    NCCLCHK(api.groupStart());
    for (int d = 0; d < N; d++) {
        Topology* T = slot_engine(top, d);
        ncclComm_t c = top->comms[(size_t)d];
        const size_t lrB = (size_t)(R * A) * sizeof(double2), hB = (size_t)(R * A) * 2;
        NCCLCHK(api.allGather((const char*)T->d_lr.p + (size_t)d * lrB, T->d_lr.p, lrB, ncclUint8, c, T->stream));
        NCCLCHK(api.allGather((const char*)T->d_hops.p + (size_t)d * hB, T->d_hops.p, hB, ncclUint8, c, T->stream));
        NCCLCHK(api.allGather(T->d_rowmin.p + (size_t)d * (size_t)R, T->d_rowmin.p, (size_t)R, ncclFloat64, c, T->stream));
    }
    NCCLCHK(api.groupEnd());
    for (int d = 0; d < N; d++) {
        Topology* T = slot_engine(top, d);
        HIPCHK(hipSetDevice(m.phys[(size_t)d]));
        HIPCHK(hipMemcpyAsync(T->d_stats.p + ST_GLOBAL_MIN, &m.dmin[(size_t)d], 8, hipMemcpyHostToDevice, T->stream));
    }
    NCCLCHK(api.groupStart());
    for (int d = 0; d < N; d++) {
        Topology* T = slot_engine(top, d);
        NCCLCHK(api.allReduce(T->d_stats.p + ST_GLOBAL_MIN, T->d_stats.p + ST_GLOBAL_MIN, 1, ncclUint64, ncclMin, top->comms[(size_t)d], T->stream));
    }
    NCCLCHK(api.groupEnd());
    for (int d = 0; d < N; d++) {
        HIPCHK(hipSetDevice(m.phys[(size_t)d]));
        HIPCHK(hipStreamSynchronize(slot_engine(top, d)->stream));
    }
    return 0;
}

// push exchange (the rows went as each shard ended): the minimum of the host's per-device minima
// to every device, blocking copies
int exchange_min_push(MultiBuild& m) {
    unsigned long long gmin = 0x7FF0000000000000ull;
    for (int d = 0; d < m.N; d++) gmin = std::min(gmin, m.dmin[(size_t)d]);
    for (int d = 0; d < m.N; d++) {
        Topology* T = slot_engine(m.top, d);
        HIPCHK(hipSetDevice(m.phys[(size_t)d]));
        HIPCHK(hipMemcpy(T->d_stats.p + ST_GLOBAL_MIN, &gmin, 8, hipMemcpyHostToDevice));
    }
    return 0;
}

}  // namespace

// N devices: slot d builds rows [d*R, min(A, (d+1)*R)) into its own full-size buffers (R*N rows,
// padded), then the rows are exchanged so that every device holds the whole table:
// ncclAllGather (in place) of the {lat, rel} rows, the u16 hop rows and the row minima, and
// ncclAllReduce(MIN) of the per-device minimum (u64 bits of a non-negative f64 order like the
// values) -> topology_getMinimumLatency / the runahead (shd-master.c:113-124).  Several slots on
// one physical device (a test configuration: RCCL refuses duplicate devices) exchange with
// device copies instead.
int build_multi(Topology* top) {
    MultiBuild m;
    m.top = top;
    const int N = m.N = std::max(1, top->devicesOpt);
    const int ndev = num_devices();
    if (ndev <= 0) {
        CRITICAL("no HIP device available: the routing engine runs on the GPU only");
        return -1;
    }
    while ((int)top->peers.size() < N - 1)
        top->peers.push_back(make_peer(top, (top->device + (int)top->peers.size() + 1) % ndev));
    for (int d = 1; d < N; d++) sync_peer(top, slot_engine(top, d));
    const int64_t A = m.A = top->A;
    const int64_t R = m.R = (A + N - 1) / N;
    top->shardRows = R;
    std::vector<int>& phys = m.phys;
    phys.resize((size_t)N);
    bool distinct = true;
    for (int d = 0; d < N; d++) {
        phys[(size_t)d] = slot_engine(top, d)->device % ndev;
        for (int e = 0; e < d; e++) distinct = distinct && phys[(size_t)e] != phys[(size_t)d];
    }
    for (int d = 0; d < N; d++) {
        int k = 0;
        for (int e = 0; e < N; e++) k += phys[(size_t)e] == phys[(size_t)d];
        slot_engine(top, d)->memShareDiv = k;
    }
    // 0) the graph is prepared once, on this engine's device, and copied to the peers
    {
        const auto tp = clk::now();
        HIPCHK(hipSetDevice(phys[0]));
        CHK(dev_init(top));
        bool did = false;
        if (!top->isComplete) {
            did = !top->csrUploaded;
            CHK(upload_csr(top));
            (void)default_delta(top);  // the mean latency, once (peers copy it)
        }
        // the peers in parallel (prepare_peer)
        std::vector<int> prc((size_t)N, 0);
        m.pdid.assign((size_t)N, 0);
        std::vector<std::thread> pth;
        for (int d = 1; d < N; d++)
            pth.emplace_back([&m, &prc, d]() { prc[(size_t)d] = prepare_peer(d, m); });
        for (auto& x : pth) x.join();
        for (int d = 1; d < N; d++) {
            if (prc[(size_t)d]) return prc[(size_t)d];
            did = did || m.pdid[(size_t)d];
        }
        HIPCHK(hipSetDevice(phys[0]));
        if (did)  // preparation + the peers' copies
            top->stats.csr_ms = std::chrono::duration<double, std::milli>(clk::now() - tp).count();
    }
    // 1) rows: device d builds rows [d R, (d+1) R) in its own host thread.
    // 2) exchange, option "exchange" (VERDICT r05 item 3):
    //    * push (2; the default for engines sharing a device): each device, as soon as its own rows
    //      are done, copies them into every other device's table on its exchange stream (peer DMA
    //      over xGMI) while the slower devices still compute -- only the last shard's copies are
    //      exposed;
    //    * rccl (1; the default for distinct devices): ncclAllGather of the rows, hops and row
    //      minima in place once every shard is done (the north-star exchange).
    //    The minimum (MIN over u64 bits of a non-negative f64 orders like the values) goes to
    //    every device -> topology_getMinimumLatency / the runahead (shd-master.c:113-124): an
    //    ncclAllReduce with RCCL, from the host's per-device minima with push.
    bool useRccl = distinct && top->xchgMode != 2;
    if (useRccl) {
        RcclApi& api = rccl();
        if (!api.ok) {
            WARNING("RCCL unavailable (%s): the rows are exchanged by peer copies", api.why.c_str());
            useRccl = false;
        } else if (top->commDevs != phys) {
            for (ncclComm_t c : top->comms) (void)api.commDestroy(c);
            top->comms.assign((size_t)N, nullptr);
            top->commDevs.clear();
            const ncclResult_t e = api.commInitAll(top->comms.data(), N, phys.data());
            if (e != ncclSuccess) {
                WARNING("ncclCommInitAll failed (%s): the rows are exchanged by peer copies",
                        api.errStr(e));
                top->comms.clear();
                useRccl = false;
            } else {
                top->commDevs = phys;
            }
        }
    }
    const bool push = m.push = !useRccl;
    // every engine's table buffers first: a device's push may arrive before the peer's own rows
    for (int d = 0; d < N; d++) {
        Topology* T = slot_engine(top, d);
        HIPCHK(hipSetDevice(phys[(size_t)d]));
        HIPCHK(T->d_lr.ensure((size_t)(R * N * A)));
        HIPCHK(T->d_hops.ensure((size_t)(R * N * A)));
        HIPCHK(T->d_rowmin.ensure((size_t)(R * N)));
        if (push && !T->xstream) HIPCHK(hipStreamCreateWithFlags(&T->xstream, hipStreamNonBlocking));
        if (push && distinct)
            for (int e = 0; e < N; e++) {
                if (e == d) continue;
                const hipError_t pe = hipDeviceEnablePeerAccess(phys[(size_t)e], 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled)
                    (void)hipGetLastError();  // no direct access: the runtime stages the copies
            }
    }
    std::vector<int> rc(N, 0);
    std::vector<double> dwall((size_t)N, 0.0);
    m.dmin.assign((size_t)N, 0x7FF0000000000000ull);
    m.drows.assign((size_t)N, 0);
    m.tdone.resize((size_t)N);
    m.tpushed.resize((size_t)N);
    const std::vector<int64_t>& drows = m.drows;
    const std::vector<clk::time_point>& tdone = m.tdone;
    const auto tb = clk::now();
    std::vector<std::thread> th;
    for (int d = 0; d < N; d++)
        th.emplace_back([&, d]() {
            rc[(size_t)d] = build_shard(d, m);
            dwall[(size_t)d] = std::chrono::duration<double, std::milli>(clk::now() - tb).count();
        });
    for (auto& x : th) x.join();
    for (int d = 0; d < N; d++)
        if (rc[(size_t)d]) return rc[(size_t)d];
    auto tfirst = tdone[0], tlast = tdone[0];
    for (int d = 1; d < N; d++) {
        tfirst = std::min(tfirst, tdone[(size_t)d]);
        tlast = std::max(tlast, tdone[(size_t)d]);
    }
    top->stats.exchange_kind = N > 1 || top->forceRccl ? (useRccl ? 1 : 2) : 0;
    top->stats.exchange_bytes = (int64_t)(N - 1) * R * (A * (int64_t)(sizeof(double2) + 2) + 8);
    CHK(useRccl ? exchange_rccl(m) : exchange_min_push(m));
    HIPCHK(hipSetDevice(phys[0]));
    auto tend = clk::now();
    if (push)
        for (int d = 0; d < N; d++) tend = std::max(tend, m.tpushed[(size_t)d]);
    const auto tx0 = useRccl ? tlast : tfirst;
    top->stats.exchange_ms = std::chrono::duration<double, std::milli>(tend - tx0).count();
    top->stats.exchange_exposed_ms = std::chrono::duration<double, std::milli>(tend - tlast).count();
    unsigned long long gm = 0;
    HIPCHK(hipMemcpy(&gm, top->d_stats.p + ST_GLOBAL_MIN, 8, hipMemcpyDeviceToHost));
    double g;
    memcpy(&g, &gm, 8);
    top->eagerMin = std::isinf(g) ? -1.0 : g;
    // whole-job statistics: the slowest device's kernels, every device's counts
    for (int d = 0; d < 8; d++) {
        top->stats.device_kernel_ms[d] = top->stats.device_build_ms[d] = 0.0;
        top->stats.device_rows[d] = 0;
    }
    for (int d = 0; d < std::min(N, 8); d++) {
        top->stats.device_kernel_ms[d] = drows[(size_t)d] > 0 ? slot_engine(top, d)->stats.build_ms : 0.0;
        top->stats.device_build_ms[d] = dwall[(size_t)d];
        top->stats.device_rows[d] = drows[(size_t)d];
    }
    top->stats.devices = N;
    top->stats.sources = A;
    for (int d = 1; d < N; d++) {
        const ShdStats& o = slot_engine(top, d)->stats;
        top->stats.sssp_kernel_ms = std::max(top->stats.sssp_kernel_ms, o.sssp_kernel_ms);
        top->stats.target_prep_ms = std::max(top->stats.target_prep_ms, o.target_prep_ms);
        top->stats.order_ms = std::max(top->stats.order_ms, o.order_ms);
        top->stats.replay_prep_ms = std::max(top->stats.replay_prep_ms, o.replay_prep_ms);
        top->stats.touched_lines += o.touched_lines;
        top->stats.replay_ms = std::max(top->stats.replay_ms, o.replay_ms);
        top->stats.build_ms = std::max(top->stats.build_ms, o.build_ms);
        top->stats.ambiguous_pairs += o.ambiguous_pairs;
        top->stats.replay_rows += o.replay_rows;
        top->stats.replay_skips += o.replay_skips;
        top->tieDense = top->tieDense || slot_engine(top, d)->tieDense;
        top->stats.errors += o.errors;
        top->stats.relaxations += o.relaxations;
    }
    return 0;
}

}  // namespace shdtopo
