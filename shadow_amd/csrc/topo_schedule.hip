// topo_schedule.hip -- route schedule for gfx950: a packet window routed through k device-resident
// A x A tables, each packet by the table that was live when it was emitted.
//
// shdtopo_route_schedule* (include/shd_topology_abi.h) is packet_route_kernel (topo_kernels.hip)
// with one more decision per packet: epoch e(i) = the largest e with from[e] <= now[i], and the
// {lat, rel} record is gathered from table e(i).  Everything after the gather is the one-table
// kernel's code, statement for statement, so a packet's outputs are the bytes that kernel gives on
// its epoch's table.  The tile is the same: 256 threads, thread t takes the packets base + j 256 +
// t for j < kRouteU, inputs loaded coalesced and nontemporal, all gathers issued before any is used.
//
//   tables   the k pointers and start times are one by-value argument (ScheduleTables): they are
//            wave-uniform and read with scalar loads in a uniform loop over e = 1 .. k - 1 that
//            compares and selects {epoch, pointer} per packet.  Nothing indexes the argument by a
//            per-lane value (that would put the arrays in scratch).
//   now      is loaded with the columns: the gather address depends on it.
//   counts   per epoch {packets, delivered, not routed} from wave ballots and popcounts into k x 3
//            LDS counters, then one global u64 atomic per non-zero counter and workgroup: exact
//            integer counts whatever the tiling.  A workgroup strides over the tiles (at most
//            kGrid workgroups per launch) and keeps its counters in LDS over all of them: with a
//            workgroup per tile a 10 M-packet window ended in 39,063 atomics on each of the same
//            few words, which took longer than the routes themselves.
//
// No thread leaves before the barriers.  Stores: t_out / state_out / delivered / epoch at k < n only,
// cnt [3 k'] for k' < t.k <= kScheduleMax; gathers at a A + b with a, b < A only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "topo_device.h"

namespace shdtopo {

namespace {

using u64 = unsigned long long;

#ifndef SHD_ROUTE_U
#define SHD_ROUTE_U 1
#endif
constexpr int kTB = 256;
constexpr int kU = SHD_ROUTE_U;  // packets per thread (gathers in flight), packet_route_kernel's
static_assert(kU >= 1 && kU <= 32, "packets per thread");
// workgroups of a launch, 16 per CU: each takes every kGrid-th tile, so a window of any size ends
// in at most kGrid atomics per global counter
constexpr int64_t kGrid = 256 * 16;

__global__ void __launch_bounds__(kTB)
route_schedule_kernel(ScheduleTables t, int64_t n, const int32_t* __restrict__ src,
                      const int32_t* __restrict__ dst, const uint32_t* __restrict__ payload,
                      const uint32_t* __restrict__ state_in, const uint64_t* __restrict__ now,
                      int64_t A, uint64_t jump, int clamp, uint64_t* __restrict__ t_out,
                      uint32_t* __restrict__ state_out, uint8_t* __restrict__ delivered,
                      uint8_t* __restrict__ epoch, u64* __restrict__ cnt) {
    __shared__ uint32_t lcnt[3 * kScheduleMax];
    if (threadIdx.x < 3 * kScheduleMax) lcnt[threadIdx.x] = 0u;
    __syncthreads();

    // a workgroup takes the tiles blk = blockIdx.x, + gridDim.x, ...: its counters stay in LDS over
    // all of them (one atomic per counter and tile on the same few global words would serialise
    // the whole launch there)
    const bool first = (threadIdx.x & 63) == 0;
    const int64_t tiles = (n + kTB * kU - 1) / (kTB * kU);
    for (int64_t blk = blockIdx.x; blk < tiles; blk += gridDim.x) {
        const int64_t tile = blk * (kTB * kU) + threadIdx.x;
        int64_t idx[kU];
        uint64_t tnow[kU];
        bool live[kU], ok[kU];
#pragma unroll
        for (int j = 0; j < kU; j++) {
            const int64_t k = tile + (int64_t)j * kTB;
            int64_t x = -1;
            tnow[j] = 0;
            live[j] = k < n;
            if (live[j]) {
                const uint32_t a = (uint32_t)__builtin_nontemporal_load(src + k);
                const uint32_t b = (uint32_t)__builtin_nontemporal_load(dst + k);
                tnow[j] = __builtin_nontemporal_load(now + k);
                if ((int64_t)a < A && (int64_t)b < A) x = (int64_t)a * A + b;
            }
            idx[j] = x;
            ok[j] = x >= 0;
        }
        // the epoch and its table: e and t.from[e] / t.lr[e] are uniform (scalar loads of the argument)
        uint32_t ep[kU];
        const double2* tab[kU];
#pragma unroll
        for (int j = 0; j < kU; j++) {
            ep[j] = 0u;
            tab[j] = t.lr[0];
        }
        for (int e = 1; e < t.k; e++) {
            const u64 from = t.from[e];
            const double2* lr = t.lr[e];
#pragma unroll
            for (int j = 0; j < kU; j++) {
                const bool at = from <= tnow[j];
                ep[j] = at ? (uint32_t)e : ep[j];
                tab[j] = at ? lr : tab[j];
            }
        }
        double2 rec[kU];
#pragma unroll
        for (int j = 0; j < kU; j++) rec[j] = ok[j] ? tab[j][idx[j]] : make_double2(0.0, -1.0);
        bool dlv[kU];
#pragma unroll
        for (int j = 0; j < kU; j++) {
            const int64_t k = tile + (int64_t)j * kTB;
            dlv[j] = false;
            if (!live[j]) continue;
            const uint32_t s0 = __builtin_nontemporal_load(state_in + k);
            const uint32_t pay = __builtin_nontemporal_load(payload + k);
            uint64_t tm = 0;
            uint8_t dl = 0;
            uint32_t next = s0;
            if (ok[j]) {
                // glibc rand_r: three LCG steps, 11 + 10 + 10 bits
                next = next * 1103515245u + 12345u;
                uint32_t r = (next / 65536u) % 2048u;
                next = next * 1103515245u + 12345u;
                r = (r << 10) ^ ((next / 65536u) % 1024u);
                next = next * 1103515245u + 12345u;
                r = (r << 10) ^ ((next / 65536u) % 1024u);
                const double chance = (double)(int32_t)r / 2147483647.0;
                if (chance <= rec[j].y || pay == 0u) {
                    const uint64_t delay = (uint64_t)ceil(rec[j].x * 1000000.0);
                    tm = tnow[j] + delay;
                    if (clamp) {
                        const uint64_t minTime = tnow[j] + jump;
                        if (tm < minTime) tm = minTime;
                    }
                    dl = 1;
                }
            }
            dlv[j] = dl != 0;
            __builtin_nontemporal_store(tm, t_out + k);
            __builtin_nontemporal_store(next, state_out + k);
            delivered[k] = dl;
            if (epoch) epoch[k] = (uint8_t)ep[j];
        }
        // the epochs' counts: ballots of 64 packets, popcounts, one LDS atomic per non-zero count
        for (int e = 0; e < t.k; e++) {
            uint32_t np = 0, nd = 0, nb = 0;
#pragma unroll
            for (int j = 0; j < kU; j++) {
                const bool in = live[j] && ep[j] == (uint32_t)e;
                const u64 m = __ballot(in);
                if (m == 0ull) continue;
                np += (uint32_t)__popcll(m);
                nd += (uint32_t)__popcll(__ballot(in && dlv[j]));
                nb += (uint32_t)__popcll(__ballot(in && !ok[j]));
            }
            if (first) {
                if (np) atomicAdd(&lcnt[3 * e], np);
                if (nd) atomicAdd(&lcnt[3 * e + 1], nd);
                if (nb) atomicAdd(&lcnt[3 * e + 2], nb);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * t.k) {
        const uint32_t v = lcnt[threadIdx.x];
        if (v) atomicAdd(cnt + threadIdx.x, (u64)v);
    }
}

}  // namespace

hipError_t launch_route_schedule(const ScheduleTables& t, int64_t n, const int32_t* src,
                                 const int32_t* dst, const uint32_t* payload,
                                 const uint32_t* state_in, const uint64_t* now, int64_t A,
                                 uint64_t jump, int clamp, uint64_t* t_out, uint32_t* state_out,
                                 uint8_t* delivered, uint8_t* epoch, unsigned long long* cnt,
                                 hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (t.k < 1 || t.k > kScheduleMax || !cnt) return hipErrorInvalidValue;
    const int64_t tiles = (n + kTB * kU - 1) / (kTB * kU);
    if (tiles > INT32_MAX) return hipErrorInvalidValue;
    const int64_t grid = tiles < kGrid ? tiles : kGrid;
    hipLaunchKernelGGL(route_schedule_kernel, dim3((unsigned)grid), dim3(kTB), 0, stream, t, n,
                       src, dst, payload, state_in, now, A, jump, clamp, t_out, state_out,
                       delivered, epoch, cnt);
    return hipGetLastError();
}

}  // namespace shdtopo
