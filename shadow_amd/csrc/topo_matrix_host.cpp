// topo_matrix_host.cpp -- the traffic matrix (include/shd_topology_abi.h shdtopo_matrix_*; kernels
// in topo_matrix.hip): an ascending vertex list mv that only grows, M x M cells of {packets,
// weight} fed by packet windows, and the export of the non-zero cells as flows.  The conventions
// are the link monitor's (topo_monitor_host.cpp): ids, the build lock, the one-event protocol of
// the device feeds, host cells for a complete topology's host feeds.
#include <arpa/inet.h>

#include "topo_host.h"

namespace shdtopo {

static_assert(sizeof(MatFlowRec) == sizeof(ShdMatrixFlow), "MatFlowRec is ShdMatrixFlow's image");

// One matrix.  The device parts appear with the first use of a device: a complete topology's host
// feeds add into h_cells and never touch one.
struct TrafficMatrix {
    std::vector<int32_t> mv;  // ascending original vertex ids; only grows
    // column -> index in mv, for the geometry it was made for (the monitor's test)
    bool mapped = false, devMap = false;
    uint64_t idxSetGen = 0, idxGeomGen = 0;
    std::vector<int32_t> idxAttached, colMap;
    DevBuf<int32_t> d_map, d_mv;
    bool devMv = false;
    // M x M cells: device (every kernel feed) and host (the host feeds of a complete topology); a
    // read that finds both adds the host cells into the device cells
    DevBuf<MatCell> d_cells;
    bool devCells = false;
    std::vector<MatCell> h_cells;
    DevBuf<unsigned long long> d_cnt;
    int64_t hcum[MX_COUNT] = {}, hlast[MX_COUNT] = {};
    int64_t unattachedCum = 0;  // of the device counters' MX_BAD: the host feeds' share
    bool lastOnDevice = false, lastHostForm = false;
    // one event: recorded by every kernel feed on its stream; ek0 / ek1 bracket the last kernel,
    // er[0..3] the passes of a read
    hipEvent_t ev = nullptr, ek0 = nullptr, ek1 = nullptr, er[4] = {};
    hipStream_t lastStream = nullptr;
    bool pending = false, timed = false;
    DevBuf<int32_t> b_src, b_dst;  // the host feeds' staging
    DevBuf<unsigned long long> b_w;
    DevBuf<uint8_t> b_dl;
    ShdMatrixStats st{};
    ~TrafficMatrix() {
        for (hipEvent_t e : {ev, ek0, ek1, er[0], er[1], er[2], er[3]})
            if (e) (void)hipEventDestroy(e);
    }
    int64_t M() const { return (int64_t)mv.size(); }
    size_t ncells() const { return mv.size() * mv.size(); }
};

std::atomic<int> g_nextMatrix{0};

TrafficMatrix* matrix_of(Topology* top, int id) {
    for (auto& m : top->matrices)
        if (m.first == id) return m.second;
    return nullptr;
}

// wait for the matrix's feeds and the library's stream
int matrix_sync(Topology* top, TrafficMatrix& m) {
    if (!top->devInit) return 0;
    HIPCHK(hipSetDevice(top->devId));
    if (m.pending) HIPCHK(hipEventSynchronize(m.ev));
    m.pending = false;
    HIPCHK(hipStreamSynchronize(top->stream));
    return 0;
}

void matrices_release(Topology* top) {
    for (auto& m : top->matrices) {
        (void)matrix_sync(top, *m.second);
        delete m.second;
    }
    top->matrices.clear();
}

// the bytes the cells may take (option "matrix_mb"); host cells have no default cap
int matrix_cap_bytes(Topology* top, bool device, double* cap) {
    *cap = 1e30;
    if (top->matrixMb > 0) {
        *cap = top->matrixMb * 1048576.0;
    } else if (device) {
        size_t fr = 0, tot = 0;
        HIPCHK(hipMemGetInfo(&fr, &tot));
        *cap = (double)fr / 2;
    }
    return 0;
}

// the device side of a matrix but its cells: events and counters (zeroed once)
int matrix_dev(Topology* top, TrafficMatrix& m) {
    CHK(dev_init(top));
    if (m.ev) return 0;
    for (hipEvent_t* e : {&m.ek0, &m.ek1, &m.er[0], &m.er[1], &m.er[2], &m.er[3]})
        if (!*e) HIPCHK(hipEventCreate(e));
    HIPCHK(m.d_cnt.ensure(2 * MX_COUNT));
    HIPCHK(hipMemset(m.d_cnt.p, 0, 8 * 2 * MX_COUNT));
    HIPCHK(hipEventCreate(&m.ev));
    return 0;
}

// Makes mv cover the current columns and colMap current.  device: the feed will use device cells.
// A growth first tests the new size against the cap, then moves every old cell of either kind.
// 0, -5 (nothing changed) or an error.
int matrix_ready(Topology* top, TrafficMatrix& m, bool device) {
    const uint64_t sg = compute_geometry(top);
    if (m.mapped && m.idxSetGen == sg && m.idxGeomGen == top->geomGen) return 0;
    if (m.mapped && m.idxAttached == top->attached) {
        m.idxSetGen = sg;  // (the set moved and came back: the same columns)
        m.idxGeomGen = top->geomGen;
        return 0;
    }
    // earlier feeds may still read the device map and the cells
    CHK(matrix_sync(top, m));
    std::vector<int32_t> nv;
    nv.reserve(m.mv.size() + top->attached.size());
    std::set_union(m.mv.begin(), m.mv.end(), top->attached.begin(), top->attached.end(),
                   std::back_inserter(nv));
    if (nv.size() != m.mv.size()) {
        const auto tstart = std::chrono::steady_clock::now();
        const int64_t M0 = m.M(), M1 = (int64_t)nv.size();
        if (M1 > 0x7FFFFFFE) return -5;
        const bool onDev = device || m.devCells;
        if (onDev) CHK(matrix_dev(top, m));
        double cap = 0;
        CHK(matrix_cap_bytes(top, onDev, &cap));
        if (16.0 * (double)M1 * (double)M1 > cap) return -5;
        std::vector<int32_t> to((size_t)M0);  // old index -> new index
        for (int64_t i = 0; i < M0; i++)
            to[(size_t)i] = (int32_t)(std::lower_bound(nv.begin(), nv.end(), m.mv[(size_t)i]) -
                                      nv.begin());
        if (m.devCells) {
            DevBuf<MatCell> nc;
            DevBuf<int32_t> d_to;
            HIPCHK(nc.ensure((size_t)M1 * (size_t)M1));
            HIPCHK(d_to.ensure((size_t)std::max<int64_t>(1, M0)));
            if (M0 > 0)
                HIPCHK(hipMemcpyAsync(d_to.p, to.data(), 4 * (size_t)M0, hipMemcpyHostToDevice,
                                      top->stream));
            HIPCHK(launch_matrix_relayout(m.d_cells.p, (int32_t)M0, d_to.p, nc.p, (int32_t)M1,
                                          top->stream));
            HIPCHK(hipStreamSynchronize(top->stream));
            std::swap(m.d_cells.p, nc.p);
            std::swap(m.d_cells.n, nc.n);
        }
        if (!m.h_cells.empty()) {
            std::vector<MatCell> nc((size_t)M1 * (size_t)M1, MatCell{0, 0});
            for (int64_t i = 0; i < M0; i++)
                for (int64_t j = 0; j < M0; j++)
                    nc[(size_t)to[(size_t)i] * (size_t)M1 + (size_t)to[(size_t)j]] =
                        m.h_cells[(size_t)(i * M0 + j)];
            m.h_cells.swap(nc);
        }
        m.mv.swap(nv);
        m.devMv = false;
        if (M0 > 0) m.st.relayouts++;
        m.st.relayout_ms = ms_since(tstart);
    }
    m.colMap.resize(top->attached.size());
    for (size_t c = 0; c < top->attached.size(); c++)
        m.colMap[c] = (int32_t)(std::lower_bound(m.mv.begin(), m.mv.end(), top->attached[c]) -
                                m.mv.begin());
    m.mapped = true;
    m.devMap = false;
    m.idxSetGen = sg;
    m.idxGeomGen = top->geomGen;
    m.idxAttached = top->attached;
    m.st.size = m.M();
    m.st.bytes = 16 * m.M() * m.M();
    return 0;
}

// device cells of the current size (zeroed when they appear) and the device map; -5: they do not
// fit the cap (tested before they are allocated)
int matrix_dev_cells(Topology* top, TrafficMatrix& m) {
    CHK(matrix_dev(top, m));
    if (!m.devCells) {
        double cap = 0;
        CHK(matrix_cap_bytes(top, true, &cap));
        if (16.0 * (double)m.ncells() > cap) return -5;
        HIPCHK(m.d_cells.ensure(std::max<size_t>(1, m.ncells())));
        HIPCHK(hipMemsetAsync(m.d_cells.p, 0, sizeof(MatCell) * std::max<size_t>(1, m.ncells()),
                              top->stream));
        HIPCHK(hipStreamSynchronize(top->stream));
        m.devCells = true;
    }
    if (!m.devMap) {
        // (matrix_ready waited for every feed that read the old map)
        HIPCHK(m.d_map.ensure(std::max<size_t>(1, m.colMap.size())));
        if (!m.colMap.empty())
            HIPCHK(hipMemcpy(m.d_map.p, m.colMap.data(), 4 * m.colMap.size(),
                             hipMemcpyHostToDevice));
        m.devMap = true;
    }
    return 0;
}

// One kernel feed on st: the matrix's stream protocol, the last feed's counters zeroed, the kernel
// between ek0 / ek1, the event recorded.  w32 or w64 carries the weights (or neither).
int matrix_launch(Topology* top, TrafficMatrix& m, const int32_t* d_src, const int32_t* d_dst,
                  const uint32_t* w32, const unsigned long long* w64, const uint8_t* d_dl,
                  int64_t n, hipStream_t st) {
    if (m.pending && st != m.lastStream) HIPCHK(hipStreamWaitEvent(st, m.ev, 0));
    const int32_t A = (int32_t)m.colMap.size(), M = (int32_t)m.M();
    HIPCHK(hipMemsetAsync(m.d_cnt.p + MX_COUNT, 0, 8 * MX_COUNT, st));
    HIPCHK(hipEventRecord(m.ek0, st));
    if (w64)
        HIPCHK(launch_matrix_feed_u64(n, d_src, d_dst, w64, d_dl, m.d_map.p, A, m.d_cells.p, M,
                                      m.d_cnt.p, st));
    else
        HIPCHK(launch_matrix_feed(n, d_src, d_dst, w32, d_dl, m.d_map.p, A, m.d_cells.p, M,
                                  m.d_cnt.p, st));
    HIPCHK(hipEventRecord(m.ek1, st));
    HIPCHK(hipEventRecord(m.ev, st));
    m.lastStream = st;
    m.pending = m.timed = true;
    m.lastOnDevice = true;
    return 0;
}

// A host feed by columns (-1: an end that is no column).  Complete topologies add into the host
// cells; the others stage the arrays, run the feed kernel and wait for it.
int64_t matrix_feed_cols(Topology* top, TrafficMatrix& m, const std::vector<int32_t>& sc,
                         const std::vector<int32_t>& dc, const uint64_t* weight,
                         const uint8_t* delivered, int64_t n) {
    m.st.feeds++;
    if (n == 0) return 0;
    CHK(matrix_ready(top, m, !top->isComplete));
    if (top->isComplete) {
        if (m.h_cells.empty()) {
            double cap = 0;
            CHK(matrix_cap_bytes(top, false, &cap));
            if (16.0 * (double)m.ncells() > cap) return -5;
            m.h_cells.assign(m.ncells(), MatCell{0, 0});
        }
        m.lastHostForm = true;
        int64_t* c = m.hlast;
        std::fill(c, c + MX_COUNT, (int64_t)0);
        const size_t M = m.mv.size();
        for (int64_t i = 0; i < n; i++) {
            if (delivered && !delivered[i]) {
                c[MX_SKIPPED]++;
                continue;
            }
            if (sc[(size_t)i] < 0 || dc[(size_t)i] < 0) {
                c[MX_BAD]++;
                continue;
            }
            c[MX_FED]++;
            MatCell& x = m.h_cells[(size_t)m.colMap[(size_t)sc[(size_t)i]] * M +
                                   (size_t)m.colMap[(size_t)dc[(size_t)i]]];
            x.packets += 1;
            x.weight += weight ? weight[i] : 1;
        }
        for (int i = 0; i < MX_COUNT; i++) m.hcum[i] += c[i];
        m.lastOnDevice = false;
        m.timed = false;
        return c[MX_FED];
    }
    CHK(matrix_dev_cells(top, m));
    m.lastHostForm = true;
    hipStream_t st = top->stream;
    const size_t nn = (size_t)n;
    HIPCHK(m.b_src.ensure(nn)); HIPCHK(m.b_dst.ensure(nn));
    HIPCHK(hipMemcpyAsync(m.b_src.p, sc.data(), 4 * nn, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(m.b_dst.p, dc.data(), 4 * nn, hipMemcpyHostToDevice, st));
    if (weight) {
        HIPCHK(m.b_w.ensure(nn));
        HIPCHK(hipMemcpyAsync(m.b_w.p, weight, 8 * nn, hipMemcpyHostToDevice, st));
    }
    if (delivered) {
        HIPCHK(m.b_dl.ensure(nn));
        HIPCHK(hipMemcpyAsync(m.b_dl.p, delivered, nn, hipMemcpyHostToDevice, st));
    }
    CHK(matrix_launch(top, m, m.b_src.p, m.b_dst.p, nullptr, weight ? m.b_w.p : nullptr,
                      delivered ? m.b_dl.p : nullptr, n, st));
    unsigned long long c[MX_COUNT] = {};
    HIPCHK(hipMemcpyAsync(c, m.d_cnt.p + MX_COUNT, 8 * MX_COUNT, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    m.pending = false;
    m.unattachedCum += (int64_t)c[MX_BAD];
    return (int64_t)c[MX_FED];
}

// a host feed by the packets' ends (IPs or vertices; vertex: an end's vertex, < 0 = none)
template <class T, class F>
int64_t matrix_feed_ends(Topology* top, int id, const T* src, const T* dst, const uint64_t* weight,
                         const uint8_t* delivered, int64_t n, F&& vertex) {
    if (!top || n < 0 || n > 0x7FFFFFFE) return -1;
    if (n > 0 && (!src || !dst)) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    TrafficMatrix* m = matrix_of(top, id);
    if (!m) return -1;
    compute_geometry(top);
    std::vector<int32_t> sc((size_t)n), dc((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int32_t s = vertex(src[i]), d = vertex(dst[i]);
        sc[(size_t)i] = s >= 0 && s < top->g.V ? top->colOf[(size_t)s] : -1;
        dc[(size_t)i] = d >= 0 && d < top->g.V ? top->colOf[(size_t)d] : -1;
    }
    return matrix_feed_cols(top, *m, sc, dc, weight, delivered, n);
}

// what a read returns besides the records, M-sized arrays on the host
struct MatrixSums {
    std::vector<uint64_t> sentP, sentW, recvP, recvW;
    ShdMatrixTotals tot{};
};

// a read answered from the host cells (or from no cells at all)
int64_t matrix_read_host(TrafficMatrix& m, ShdMatrixFlow* out, int64_t cap, MatrixSums& s) {
    const int64_t M = m.M();
    std::vector<uint8_t> act((size_t)M, 0);
    ShdMatrixTotals& t = s.tot;
    int64_t total = 0;
    if (m.h_cells.empty()) return 0;
    for (int64_t i = 0; i < M; i++) {
        bool any = false;
        for (int64_t j = 0; j < M; j++) {
            const MatCell& c = m.h_cells[(size_t)(i * M + j)];
            if (!(c.packets | c.weight)) continue;
            any = true;
            act[(size_t)j] = 1;
            s.sentP[(size_t)i] += c.packets;
            s.sentW[(size_t)i] += c.weight;
            s.recvP[(size_t)j] += c.packets;
            s.recvW[(size_t)j] += c.weight;
            t.packets += c.packets;
            t.weight += c.weight;
            if (i == j) {
                t.selfCells++;
                t.selfPackets += c.packets;
                t.selfWeight += c.weight;
            }
            if (t.peakCell < 0 || c.weight > t.peakWeight) {  // (ascending: the lowest index stays)
                t.peakWeight = c.weight;
                t.peakCell = i * M + j;
            }
            if (total < cap && out)
                out[total] = ShdMatrixFlow{m.mv[(size_t)i], m.mv[(size_t)j], (int32_t)i, (int32_t)j,
                                           c.packets, c.weight};
            total++;
        }
        if (any) t.activeSources++;
    }
    for (uint8_t a : act) t.activeDestinations += a;
    t.cells = total;
    return total;
}

// a read of the device cells: count, scan, fill
int64_t matrix_read_dev(Topology* top, TrafficMatrix& m, ShdMatrixFlow* out, int64_t cap,
                        MatrixSums& s) {
    const int64_t M = m.M();
    const size_t MM = (size_t)M;
    hipStream_t st = top->stream;
    if (!m.h_cells.empty()) {
        // both kinds of cells: the host cells are added into the device cells and cleared
        DevBuf<MatCell> up;
        HIPCHK(up.ensure(m.ncells()));
        HIPCHK(hipMemcpyAsync(up.p, m.h_cells.data(), sizeof(MatCell) * m.ncells(),
                              hipMemcpyHostToDevice, st));
        HIPCHK(launch_matrix_add(m.d_cells.p, up.p, (int64_t)m.ncells(), st));
        HIPCHK(hipStreamSynchronize(st));
        std::vector<MatCell>().swap(m.h_cells);
    }
    if (!m.devMv) {
        HIPCHK(m.d_mv.ensure(MM));
        HIPCHK(hipMemcpy(m.d_mv.p, m.mv.data(), 4 * MM, hipMemcpyHostToDevice));
        m.devMv = true;
    }
    // one block of u64 words: sentP, sentW, recvP, recvW, rowPeakW [M each], tot; the i64 arrays
    // rowCells, rowOff [M + 1 each], rowPeakCell [M]; colActive u32 [M]
    DevBuf<unsigned long long> d_u;
    DevBuf<int64_t> d_i;
    DevBuf<uint32_t> d_act;
    HIPCHK(d_u.ensure(5 * MM + MT_COUNT));
    HIPCHK(d_i.ensure(3 * MM + 2));
    HIPCHK(d_act.ensure(MM));
    HIPCHK(hipMemsetAsync(d_u.p, 0, 8 * (5 * MM + MT_COUNT), st));
    HIPCHK(hipMemsetAsync(d_i.p, 0, 8 * (3 * MM + 2), st));
    HIPCHK(hipMemsetAsync(d_act.p, 0, 4 * MM, st));
    MatCount o;
    o.sentP = d_u.p;
    o.sentW = d_u.p + MM;
    o.recvP = d_u.p + 2 * MM;
    o.recvW = d_u.p + 3 * MM;
    o.rowPeakW = d_u.p + 4 * MM;
    o.tot = d_u.p + 5 * MM;
    o.rowCells = d_i.p;
    int64_t* rowOff = d_i.p + MM + 1;
    o.rowPeakCell = d_i.p + 2 * MM + 2;
    o.colActive = d_act.p;
    HIPCHK(hipEventRecord(m.er[0], st));
    HIPCHK(launch_matrix_count(m.d_cells.p, (int32_t)M, o, st));
    HIPCHK(trace_exclusive_scan(o.rowCells, rowOff, M + 1, st));
    HIPCHK(hipEventRecord(m.er[1], st));
    std::vector<unsigned long long> hu(5 * MM + MT_COUNT);
    std::vector<int64_t> hpc(MM);
    std::vector<uint32_t> hact(MM);
    int64_t total = 0;
    HIPCHK(hipMemcpyAsync(hu.data(), d_u.p, 8 * hu.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hpc.data(), o.rowPeakCell, 8 * MM, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hact.data(), d_act.p, 4 * MM, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&total, rowOff + M, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t nout = out ? std::min(total, cap) : 0;
    float ms0 = 0, ms1 = 0;
    HIPCHK(hipEventElapsedTime(&ms0, m.er[0], m.er[1]));
    int64_t walked = 0;
    if (nout > 0) {
        DevBuf<MatFlowRec> d_out;
        HIPCHK(d_out.ensure((size_t)nout));
        HIPCHK(hipEventRecord(m.er[2], st));
        HIPCHK(launch_matrix_fill(m.d_cells.p, (int32_t)M, m.d_mv.p, o.rowCells, rowOff, d_out.p,
                                  nout, st));
        HIPCHK(hipEventRecord(m.er[3], st));
        HIPCHK(hipMemcpyAsync(out, d_out.p, sizeof(MatFlowRec) * (size_t)nout,
                              hipMemcpyDeviceToHost, st));
        std::vector<int64_t> hoff(MM + 1);
        HIPCHK(hipMemcpyAsync(hoff.data(), rowOff, 8 * (MM + 1), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipEventElapsedTime(&ms1, m.er[2], m.er[3]));
        for (size_t i = 0; i < MM; i++)  // the rows the fill walked
            walked += hoff[i + 1] > hoff[i] && hoff[i] < nout;
    }
    m.st.read_kernel_ms = (double)ms0 + (double)ms1;
    m.st.bytes_model = 16 * M * M + 16 * M * walked + 32 * nout;
    std::copy(hu.begin(), hu.begin() + (std::ptrdiff_t)MM, s.sentP.begin());
    std::copy(hu.begin() + (std::ptrdiff_t)MM, hu.begin() + (std::ptrdiff_t)(2 * MM),
              s.sentW.begin());
    std::copy(hu.begin() + (std::ptrdiff_t)(2 * MM), hu.begin() + (std::ptrdiff_t)(3 * MM),
              s.recvP.begin());
    std::copy(hu.begin() + (std::ptrdiff_t)(3 * MM), hu.begin() + (std::ptrdiff_t)(4 * MM),
              s.recvW.begin());
    const unsigned long long* tt = hu.data() + 5 * MM;
    ShdMatrixTotals& t = s.tot;
    t.cells = (int64_t)tt[MT_CELLS];
    t.packets = tt[MT_PACKETS];
    t.weight = tt[MT_WEIGHT];
    t.selfCells = (int64_t)tt[MT_SELF_CELLS];
    t.selfPackets = tt[MT_SELF_PACKETS];
    t.selfWeight = tt[MT_SELF_WEIGHT];
    t.activeSources = (int64_t)tt[MT_ACTIVE_SRC];
    for (size_t i = 0; i < MM; i++) {
        t.activeDestinations += hact[i] != 0;
        const uint64_t pw = hu[4 * MM + i];
        if (hpc[i] >= 0 && (t.peakCell < 0 || pw > t.peakWeight)) {  // (rows ascend)
            t.peakWeight = pw;
            t.peakCell = hpc[i];
        }
    }
    return total;
}

}  // namespace shdtopo

extern "C" {

int shdtopo_matrix_new(Topology* top) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    const int id = g_nextMatrix.fetch_add(1);
    top->matrices.emplace_back(id, new TrafficMatrix());
    return id;
}

int shdtopo_matrix_free(Topology* top, int id) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    for (size_t k = 0; k < top->matrices.size(); k++)
        if (top->matrices[k].first == id) {
            (void)matrix_sync(top, *top->matrices[k].second);
            delete top->matrices[k].second;
            top->matrices.erase(top->matrices.begin() + (std::ptrdiff_t)k);
            return 0;
        }
    return -1;
}

int64_t shdtopo_matrix_feed(Topology* top, int id, const uint32_t* srcIP, const uint32_t* dstIP,
                            const uint64_t* weight, const uint8_t* delivered, int64_t n) {
    return matrix_feed_ends(top, id, srcIP, dstIP, weight, delivered, n,
                            [&](uint32_t ip) { return vertex_of_ip(top, ip); });
}

int64_t shdtopo_matrix_feed_vertices(Topology* top, int id, const int32_t* srcVertex,
                                     const int32_t* dstVertex, const uint64_t* weight,
                                     const uint8_t* delivered, int64_t n) {
    return matrix_feed_ends(top, id, srcVertex, dstVertex, weight, delivered, n,
                            [](int32_t v) { return v; });
}

int shdtopo_matrix_feed_device(Topology* top, int id, const int32_t* d_srcCol,
                               const int32_t* d_dstCol, const uint32_t* d_payload,
                               const uint8_t* d_delivered, int64_t n, void* stream) {
    if (!top || n < 0 || n > 0x7FFFFFFE) return -1;
    if (n > 0 && (!d_srcCol || !d_dstCol)) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    TrafficMatrix* m = matrix_of(top, id);
    if (!m) return -1;
    m->st.feeds++;
    if (n == 0) return 0;
    CHK(matrix_ready(top, *m, true));
    CHK(matrix_dev_cells(top, *m));
    m->lastHostForm = false;
    hipStream_t st = stream ? (hipStream_t)stream : top->stream;
    return matrix_launch(top, *m, d_srcCol, d_dstCol, d_payload, nullptr, d_delivered, n, st);
}

int64_t shdtopo_matrix_vertices(Topology* top, int id, int32_t* out, int64_t cap) {
    if (!top || cap < 0) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    TrafficMatrix* m = matrix_of(top, id);
    if (!m) return -1;
    CHK(matrix_sync(top, *m));
    if (out) std::copy(m->mv.begin(), m->mv.begin() + (std::ptrdiff_t)std::min(cap, m->M()), out);
    return m->M();
}

int64_t shdtopo_matrix_read(Topology* top, int id, ShdMatrixFlow* out, int64_t cap,
                            uint64_t* sentPackets, uint64_t* sentWeight, uint64_t* recvPackets,
                            uint64_t* recvWeight, ShdMatrixTotals* totals) {
    if (!top || cap < 0 || (cap > 0 && !out)) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    TrafficMatrix* m = matrix_of(top, id);
    if (!m) return -1;
    const auto tstart = std::chrono::steady_clock::now();
    CHK(matrix_sync(top, *m));
    const size_t M = m->mv.size();
    MatrixSums s;
    s.sentP.assign(M, 0); s.sentW.assign(M, 0); s.recvP.assign(M, 0); s.recvW.assign(M, 0);
    s.tot.size = (int64_t)M;
    s.tot.peakCell = -1;
    int64_t total = 0;
    m->st.read_kernel_ms = 0;
    if (m->devCells && M > 0) {
        total = matrix_read_dev(top, *m, out, cap, s);
    } else {
        total = matrix_read_host(*m, out, cap, s);
        m->st.bytes_model = 0;
    }
    if (total < 0) return total;
    if (sentPackets) std::copy(s.sentP.begin(), s.sentP.end(), sentPackets);
    if (sentWeight) std::copy(s.sentW.begin(), s.sentW.end(), sentWeight);
    if (recvPackets) std::copy(s.recvP.begin(), s.recvP.end(), recvPackets);
    if (recvWeight) std::copy(s.recvW.begin(), s.recvW.end(), recvWeight);
    if (totals) *totals = s.tot;
    m->st.cells = total;
    m->st.read_ms = ms_since(tstart);
    return total;
}

int shdtopo_matrix_reset(Topology* top, int id) {
    if (!top) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    TrafficMatrix* m = matrix_of(top, id);
    if (!m) return -1;
    CHK(matrix_sync(top, *m));
    if (m->devCells)
        HIPCHK(hipMemsetAsync(m->d_cells.p, 0, sizeof(MatCell) * std::max<size_t>(1, m->ncells()),
                              top->stream));
    if (m->d_cnt.p) HIPCHK(hipMemsetAsync(m->d_cnt.p, 0, 8 * 2 * MX_COUNT, top->stream));
    if (m->devCells || m->d_cnt.p) HIPCHK(hipStreamSynchronize(top->stream));
    std::fill(m->h_cells.begin(), m->h_cells.end(), MatCell{0, 0});
    std::fill(m->hcum, m->hcum + MX_COUNT, (int64_t)0);
    std::fill(m->hlast, m->hlast + MX_COUNT, (int64_t)0);
    m->unattachedCum = 0;
    return 0;
}

int shdtopo_matrix_stats(Topology* top, int id, ShdMatrixStats* out) {
    if (!top || !out) return -1;
    std::lock_guard<std::mutex> lk(top->buildMu);
    TrafficMatrix* m = matrix_of(top, id);
    if (!m) return -1;
    CHK(matrix_sync(top, *m));
    unsigned long long dc[2 * MX_COUNT] = {};
    if (m->d_cnt.p) HIPCHK(hipMemcpy(dc, m->d_cnt.p, sizeof dc, hipMemcpyDeviceToHost));
    ShdMatrixStats& s = m->st;
    if (m->timed) {  // taken lazily: the feed itself never waits
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, m->ek0, m->ek1));
        s.feed_kernel_ms = ms;
    } else {
        s.feed_kernel_ms = 0;
    }
    s.fed = m->hcum[MX_FED] + (int64_t)dc[MX_FED];
    s.skipped_undelivered = m->hcum[MX_SKIPPED] + (int64_t)dc[MX_SKIPPED];
    s.unattached = m->hcum[MX_BAD] + m->unattachedCum;
    s.bad_columns = (int64_t)dc[MX_BAD] - m->unattachedCum;
    auto last = [&](int i) {
        return m->lastOnDevice ? (int64_t)dc[MX_COUNT + i] : m->hlast[i];
    };
    s.last_fed = last(MX_FED);
    s.last_skipped_undelivered = last(MX_SKIPPED);
    s.last_unattached = m->lastHostForm ? last(MX_BAD) : 0;
    s.last_bad_columns = m->lastHostForm ? 0 : last(MX_BAD);
    s.size = m->M();
    s.bytes = 16 * m->M() * m->M();
    *out = s;
    return 0;
}

int64_t shdtopo_vertex_ips(Topology* top, const int32_t* vertex, int64_t n, uint32_t* ip) {
    if (!top || n < 0 || (n > 0 && (!vertex || !ip))) return -1;
    const int64_t V = top->g.V;
    for (int64_t i = 0; i < n; i++)
        if (vertex[i] < 0 || vertex[i] >= V) return -1;
    // per requested vertex its lowest IP in host byte order (0: none yet)
    std::unordered_map<int32_t, uint64_t> low;
    low.reserve((size_t)n * 2);
    for (int64_t i = 0; i < n; i++) low.emplace(vertex[i], UINT64_MAX);
    {
        std::shared_lock<std::shared_mutex> lk(top->ipMu);
        for (const auto& kv : top->virtualIP) {
            const auto it = low.find(kv.second);
            if (it == low.end()) continue;
            const uint64_t h = ntohl(kv.first);
            if (h < it->second) it->second = h;
        }
    }
    int64_t got = 0;
    for (int64_t i = 0; i < n; i++) {
        const uint64_t h = low[vertex[i]];
        ip[i] = h == UINT64_MAX ? 0u : htonl((uint32_t)h);
        got += h != UINT64_MAX;
    }
    return got;
}

}  // extern "C"
