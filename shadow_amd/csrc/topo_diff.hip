// topo_diff.hip -- table diff for gfx950: what changed between two device-resident A x A tables.
//
// shdtopo_table_diff (include/shd_topology_abi.h) compares the {latency, reliability} records
// and the u16 hop counts of two topologies with the same attached vertices, pair by pair, and
// returns only the changed pairs -- the tables themselves (2 x 1.8 GB at 10,000 columns) never
// leave the device.
//
//   count  one 256-thread workgroup per row s: thread t takes the columns t, t + 256, ... so a
//          wavefront reads 64 consecutive 16-B records of each table (1 KiB per load instruction)
//          and 64 consecutive u16 hops; a pair is changed when the latency bits, the reliability
//          bits or the hops differ.  The row's changed pairs go to rowChanged[s] (i64, the scan's
//          input), its largest latency rise and the lowest column reaching it to rowWorstRise /
//          rowWorstCol, the four kind bits' pair counts to kindCount (one u64 atomic per bit and
//          workgroup with a non-zero count: integer sums, any order gives the same result);
//   scan   trace_exclusive_scan over rowChanged: each row's first record;
//   fill   the same walk over the rows that have a change and start below the caller's cap: per
//          256-column step a wave ballot and prefix popcount number the changed pairs of a
//          wavefront, the four wave totals are combined through LDS, and every changed pair writes
//          its 48-B record (three 16-B stores) at rowOffset + its rank: row-major order, column
//          ascending within the row, with no sort and no atomic.
//
// Streaming: 36 B read per pair and pass (2 x 16 B records, 2 x 2 B hops); rows without a change
// are not read a second time.  No kernel stores outside rowChanged / rowWorst* [A], kindCount [4]
// and out[min(total, cap)]: every index is bounded by s < A, d < A or pos < cap.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "topo_dev_common.h"
#include "topo_paircmp.h"

namespace shdtopo {

namespace {

using namespace dev;
using u64 = unsigned long long;

constexpr int kTB = 256;
constexpr int kNW = kTB / 64;

static_assert(sizeof(DiffRec) == 48, "DiffRec is three 16-B stores");

__global__ __launch_bounds__(kTB) void diff_count_kernel(DiffTables t, int64_t* rowChanged,
                                                         double* rowWorstRise,
                                                         int32_t* rowWorstCol, u64* kindCount) {
    __shared__ uint32_t s_cnt[5];
    __shared__ double s_rise[kNW];
    __shared__ int32_t s_col[kNW];
    const int32_t A = t.A;
    const int64_t s = blockIdx.x;  // grid = A
    const size_t base = (size_t)s * (size_t)A;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x < 5) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t changed = 0, kc[4] = {0, 0, 0, 0};
    double rise = 0.0;
    int32_t col = -1;
    for (int32_t d = (int32_t)threadIdx.x; d < A; d += kTB) {
        const double2 x0 = t.lr0[base + (size_t)d], x1 = t.lr1[base + (size_t)d];
        const uint32_t h0 = t.hops0[base + (size_t)d], h1 = t.hops1[base + (size_t)d];
        if (!pair_changed(x0, x1, h0, h1)) continue;
        changed++;
        const uint32_t k = pair_kind(x0, x1, h0, h1);
#pragma unroll
        for (int i = 0; i < 4; i++) kc[i] += (k >> i) & 1u;
        if (k & kDiffLatRose) {
            const double r = x1.x - x0.x;
            if (r > rise) {  // a thread's columns ascend: the first one to reach the maximum stays
                rise = r;
                col = d;
            }
        }
    }
    // the wavefront's sums and its {largest rise, lowest column}
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        changed += __shfl_xor(changed, o, 64);
#pragma unroll
        for (int i = 0; i < 4; i++) kc[i] += __shfl_xor(kc[i], o, 64);
    }
    wave_worst_rise(rise, col);
    if (lane == 0) {
        if (changed) atomicAdd(&s_cnt[4], changed);
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (kc[i]) atomicAdd(&s_cnt[i], kc[i]);
        s_rise[wid] = rise;
        s_col[wid] = col;
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&kindCount[threadIdx.x], (u64)s_cnt[threadIdx.x]);
    if (threadIdx.x == 0) {
        for (int w = 1; w < kNW; w++) {
            const double r = s_rise[w];
            const int32_t c = s_col[w];
            if (worse_rise(r, c, rise, col)) {
                rise = r;
                col = c;
            }
        }
        rowChanged[s] = (int64_t)s_cnt[4];
        rowWorstRise[s] = col >= 0 ? rise : 0.0;
        rowWorstCol[s] = col;
    }
}

__global__ __launch_bounds__(kTB) void diff_fill_kernel(DiffTables t, const int64_t* rowChanged,
                                                        const int64_t* rowOff, DiffRec* out,
                                                        int64_t cap) {
    __shared__ uint32_t s_wave[kNW];
    const int32_t A = t.A;
    const int64_t s = blockIdx.x;  // grid = A
    // (both conditions are the same for every thread of the workgroup)
    if (rowChanged[s] == 0) return;
    int64_t pos = rowOff[s];
    if (pos >= cap) return;
    const size_t base = (size_t)s * (size_t)A;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int32_t d0 = 0; d0 < A; d0 += kTB) {
        const int32_t d = d0 + (int32_t)threadIdx.x;
        double2 x0{0.0, 0.0}, x1{0.0, 0.0};
        uint32_t h0 = 0, h1 = 0;
        bool ch = false;
        if (d < A) {
            x0 = t.lr0[base + (size_t)d];
            x1 = t.lr1[base + (size_t)d];
            h0 = t.hops0[base + (size_t)d];
            h1 = t.hops1[base + (size_t)d];
            ch = pair_changed(x0, x1, h0, h1);
        }
        const u64 m = __ballot(ch);
        if (lane == 0) s_wave[wid] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kNW; w++) {
            const uint32_t c = s_wave[w];
            before += w < wid ? c : 0u;
            all += c;
        }
        if (ch) {
            const int64_t p = pos + (int64_t)before + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
            if (p < cap) {
                DiffRec r;
                r.srcCol = (int32_t)s;
                r.dstCol = d;
                r.lat0 = x0.x;
                r.lat1 = x1.x;
                r.rel0 = x0.y;
                r.rel1 = x1.y;
                r.hops = (h0 & 0xFFFFu) | (h1 << 16);
                r.kind = pair_kind(x0, x1, h0, h1);
                out[p] = r;
            }
        }
        pos += (int64_t)all;
        if (pos >= cap) return;  // (uniform: pos is the same in every thread)
        __syncthreads();         // s_wave is rewritten by the next step
    }
}

}  // namespace

hipError_t launch_diff_count(const DiffTables& t, int64_t* rowChanged, double* rowWorstRise,
                             int32_t* rowWorstCol, unsigned long long* kindCount,
                             hipStream_t stream) {
    if (t.A <= 0) return hipSuccess;
    if (!t.lr0 || !t.lr1 || !t.hops0 || !t.hops1 || !rowChanged || !rowWorstRise ||
        !rowWorstCol || !kindCount)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(diff_count_kernel, dim3((unsigned)t.A), dim3(kTB), 0, stream, t, rowChanged,
                       rowWorstRise, rowWorstCol, kindCount);
    return hipGetLastError();
}

hipError_t launch_diff_fill(const DiffTables& t, const int64_t* rowChanged, const int64_t* rowOff,
                            DiffRec* out, int64_t cap, hipStream_t stream) {
    if (t.A <= 0 || cap <= 0) return hipSuccess;
    if (!t.lr0 || !t.lr1 || !t.hops0 || !t.hops1 || !rowChanged || !rowOff || !out)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(diff_fill_kernel, dim3((unsigned)t.A), dim3(kTB), 0, stream, t, rowChanged,
                       rowOff, out, cap);
    return hipGetLastError();
}

}  // namespace shdtopo
