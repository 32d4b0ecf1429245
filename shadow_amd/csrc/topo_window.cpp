// topo_window.cpp -- the engine-side window adapter (include/shd_topology_window.h, SURVEY.md
// 8(f)#3): worker_schedulePacket (src/engine/shd-worker.c:332-370) recorded at emit and routed
// as one GPU batch at the scheduler's window barrier (shd-slave.c:415-461).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/shd_topology_window.h"
#include "topo_host.h"

extern "C" {
__attribute__((weak)) uint32_t address_toNetworkIP(Address* address);
__attribute__((weak)) double random_nextDouble(Random* random);
}

// One recorded packet: its vertices are resolved at emit, when the reference routed it
// (shd-worker.c:345-369), so a host detached before the flush does not lose its packets.
struct WinPacket {
    int32_t srcV, dstV;
    uint32_t payloadLength, rngState;
    uint64_t now;
    void* packet;
};

struct _TopoWindow {
    Topology* top = nullptr;
    std::mutex mu;  // worker threads emit concurrently; the window keeps their real-time order
    std::vector<WinPacket> in;
    std::vector<TopoPacketOut> out;
    int monitor = -1;         // topowindow_set_monitor: the link monitor fed at every flush
    bool monitorBytes = true;  // its weight: payloadLength, else 1 per packet
    int matrix = -1;          // topowindow_set_matrix: the traffic matrix fed at every flush
    bool matrixBytes = true;   // its weight: payloadLength, else 1 per packet
    // topowindow_set_schedule: the members and start times every flush routes through (empty:
    // none; sched[0] == top), and the distinct members besides top, each held by one
    // shdtopo_window_hold(+1)
    std::vector<Topology*> sched;
    std::vector<uint64_t> schedFrom;
    std::vector<Topology*> schedHeld;
};

namespace {
// drop the holds of a schedule's other members; a column one kept for the window may go, unless
// the member is held again by the schedule that follows (keep)
void drop_schedule_holds(std::vector<Topology*>& held, const std::vector<Topology*>& keep = {}) {
    for (Topology* m : held) {
        shdtopo_window_hold(m, -1);
        if (std::find(keep.begin(), keep.end(), m) == keep.end()) shdtopo_window_release(m);
    }
    held.clear();
}
}  // namespace

extern "C" {

TopoWindow* topowindow_new(Topology* top) {
    if (!top) return nullptr;
    TopoWindow* w = new TopoWindow();
    w->top = top;
    shdtopo_window_hold(top, +1);
    return w;
}

void topowindow_free(TopoWindow* w) {
    if (!w) return;
    drop_schedule_holds(w->schedHeld);
    shdtopo_window_hold(w->top, -1);
    shdtopo_window_release(w->top);
    delete w;
}

int64_t topowindow_emit_state(TopoWindow* w, uint32_t srcIP, uint32_t dstIP,
                              uint32_t payloadLength, uint32_t preDrawState, uint64_t now,
                              void* packet) {
    if (!w) return -1;
    // the reference's getters return -1.0 for an address the topology does not know (the
    // packet is then dropped unless a control packet): not routed here, the caller drops it
    const int32_t sv = shdtopo_vertex_of_ip(w->top, srcIP), dv = shdtopo_vertex_of_ip(w->top, dstIP);
    if (sv < 0 || dv < 0) return -1;
    std::lock_guard<std::mutex> lk(w->mu);
    w->in.push_back(WinPacket{sv, dv, payloadLength, preDrawState, now, packet});
    return (int64_t)w->in.size() - 1;
}

int64_t topowindow_emit(TopoWindow* w, Address* src, Address* dst, uint32_t payloadLength,
                        Random* senderRandom, uint64_t now, void* packet) {
    if (!w || !src || !dst || !senderRandom || !address_toNetworkIP || !random_nextDouble)
        return -1;
    // Shadow's Random is { guint seedState; guint initialSeed; } (shd-random.c:13-16): the state
    // before the reference's one draw (shd-worker.c:353-354), then that draw on the stream
    uint32_t pre;
    memcpy(&pre, (const void*)senderRandom, sizeof pre);
    (void)random_nextDouble(senderRandom);
    return topowindow_emit_state(w, address_toNetworkIP(src), address_toNetworkIP(dst),
                                 payloadLength, pre, now, packet);
}

int64_t topowindow_pending(TopoWindow* w) {
    if (!w) return -1;
    std::lock_guard<std::mutex> lk(w->mu);
    return (int64_t)w->in.size();
}

int topowindow_set_monitor(TopoWindow* w, int monitor, int bytes) {
    if (!w) return -1;
    std::lock_guard<std::mutex> lk(w->mu);
    w->monitor = monitor < 0 ? -1 : monitor;
    w->monitorBytes = bytes != 0;
    return 0;
}

int topowindow_set_matrix(TopoWindow* w, int matrix, int bytes) {
    if (!w) return -1;
    std::lock_guard<std::mutex> lk(w->mu);
    w->matrix = matrix < 0 ? -1 : matrix;
    w->matrixBytes = bytes != 0;
    return 0;
}

int topowindow_set_schedule(TopoWindow* w, Topology* const* tops, const uint64_t* fromNs, int k) {
    if (!w || k < 0 || k > SHD_SCHEDULE_MAX) return -1;
    std::vector<Topology*> sched, held;
    std::vector<uint64_t> from;
    if (k > 0) {
        if (!tops || !fromNs || tops[0] != w->top || fromNs[0] != 0) return -1;
        for (int e = 0; e < k; e++)
            if (!tops[e] || (e > 0 && fromNs[e] <= fromNs[e - 1])) return -1;
        sched.assign(tops, tops + k);
        from.assign(fromNs, fromNs + k);
        for (Topology* m : sched)
            if (m != w->top && std::find(held.begin(), held.end(), m) == held.end())
                held.push_back(m);
    }
    // the new members are held before the old ones are let go: one that is in both keeps its
    // deferred columns
    for (Topology* m : held) shdtopo_window_hold(m, +1);
    std::lock_guard<std::mutex> lk(w->mu);
    drop_schedule_holds(w->schedHeld, held);
    w->sched.swap(sched);
    w->schedFrom.swap(from);
    w->schedHeld.swap(held);
    return 0;
}

int topowindow_flush(TopoWindow* w, uint64_t jumpNs, int multiThreaded, TopoWindowDeliver deliver,
                     void* ctx) {
    if (!w) return -1;
    std::vector<WinPacket> in;
    std::vector<Topology*> sched, held;
    std::vector<uint64_t> from;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        in.swap(w->in);
        sched = w->sched;
        from = w->schedFrom;
        held = w->schedHeld;
    }
    if (in.empty()) {
        shdtopo_window_release(w->top);
        for (Topology* m : held) shdtopo_window_release(m);
        return 0;
    }
    const size_t n = in.size();
    std::vector<int32_t> sv(n), dv(n);
    std::vector<uint32_t> pay(n), st(n);
    std::vector<uint64_t> now(n);
    for (size_t i = 0; i < n; i++) {
        sv[i] = in[i].srcV;
        dv[i] = in[i].dstV;
        pay[i] = in[i].payloadLength;
        st[i] = in[i].rngState;
        now[i] = in[i].now;
    }
    w->out.resize(n);
    // a vertex detached during the window is still a column (shdtopo_window_hold): its packets
    // are routed as at emit; only a packet whose vertex left before an earlier flush comes back
    // undelivered
    // (under a schedule each packet by the member live at its emission time; the members hold the
    // same columns: the caller mirrors attach and detach on all of them)
    const int64_t r =
        sched.empty()
            ? shdtopo_route_batch_vertices(w->top, sv.data(), dv.data(), pay.data(), st.data(),
                                           now.data(), n, jumpNs, multiThreaded, w->out.data())
            : shdtopo_route_schedule_vertices(sched.data(), from.data(), (int)sched.size(),
                                              sv.data(), dv.data(), pay.data(), st.data(),
                                              now.data(), (int64_t)n, jumpNs, multiThreaded,
                                              w->out.data(), nullptr, nullptr);
    if (r < 0) {
        // nothing was routed: the window is put back in front of what was emitted meanwhile, so
        // a later flush routes every packet in emission order
        std::lock_guard<std::mutex> lk(w->mu);
        in.insert(in.end(), w->in.begin(), w->in.end());
        w->in.swap(in);
        return (int)r;
    }
    // the link monitor and the traffic matrix see the window before its deferred columns go: the
    // packets the batch delivered, at their emission times.  A feed error costs the monitor or the
    // matrix the window, not the run.
    int monitor, matrix;
    bool bytes, mbytes;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        monitor = w->monitor;
        bytes = w->monitorBytes;
        matrix = w->matrix;
        mbytes = w->matrixBytes;
    }
    std::vector<uint64_t> wt;
    std::vector<uint8_t> dl;
    if (monitor >= 0 || matrix >= 0) {
        dl.resize(n);
        if ((monitor >= 0 && bytes) || (matrix >= 0 && mbytes)) wt.assign(pay.begin(), pay.end());
        for (size_t i = 0; i < n; i++) dl[i] = w->out[i].delivered ? 1 : 0;
    }
    if (monitor >= 0) {
        const int64_t fr = shdtopo_monitor_feed_vertices(w->top, monitor, sv.data(), dv.data(),
                                                         bytes ? wt.data() : nullptr, now.data(),
                                                         dl.data(), (int64_t)n);
        if (fr < 0)
            WARNING("link monitor %d: feeding a window of %lld packets failed: %lld", monitor,
                    (long long)n, (long long)fr);
    }
    if (matrix >= 0) {
        const int64_t fr = shdtopo_matrix_feed_vertices(w->top, matrix, sv.data(), dv.data(),
                                                        mbytes ? wt.data() : nullptr, dl.data(),
                                                        (int64_t)n);
        if (fr < 0)
            WARNING("traffic matrix %d: feeding a window of %lld packets failed: %lld", matrix,
                    (long long)n, (long long)fr);
    }
    // the window's packets are routed: vertices detached during it may leave the table now
    shdtopo_window_release(w->top);
    for (Topology* m : held) shdtopo_window_release(m);
    if (deliver)
        for (size_t i = 0; i < n; i++)
            deliver(ctx, in[i].packet, w->out[i].delivered, w->out[i].time);
    return 0;
}

uint64_t topowindow_jump_ns(Topology* top, uint64_t runaheadNs) {
    const double m = topology_getMinimumLatency(top);
    uint64_t jump = m > 0 ? ((uint64_t)m) * 1000000ull : 0;  // shd-master.c:118
    if (jump == 0) jump = 10ull * 1000000ull;                 // shd-master.c:103
    if (runaheadNs > 0 && jump < runaheadNs) jump = runaheadNs;  // :106-108
    return jump;
}

uint64_t topowindow_serial_window_ns(Topology* top) {
    const double m = topology_getMinimumLatency(top);
    const double ns = m > 0 ? std::floor(m * 1000000.0) : 0.0;
    return ns >= 1.0 ? (uint64_t)ns : 1ull;
}

}  // extern "C"
