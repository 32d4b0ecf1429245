// topo_matrix.hip -- traffic matrix for gfx950: packet windows summed into per-pair flows.
//
// A traffic matrix (include/shd_topology_abi.h, "traffic matrix") keeps M x M cells of 16 B,
// {u64 packets, u64 weight}, in HBM across calls: row = source vertex, column = destination vertex
// of the matrix's own ascending vertex list mv.  It walks no route and reads no table: a packet's
// cell follows from its two columns through colMap (i32[A]: column -> index in mv).
//
//   feed      one packet per thread and round: non-temporal loads of the packet arrays, two
//             gathers into colMap (40 KB at A = 10,000: cache-resident), two u64 atomicAdds on
//             the adjacent words of the cell (one line); the counters are summed per wavefront
//             and added with one atomic per counter and wave.  No LDS, no scratch;
//   relayout  a growth: old cell (i, j) goes to (map[i], map[j]) of the zeroed new matrix with one
//             16-B load and one 16-B store;
//   add       a read that finds host cells beside the device cells adds the uploaded host cells;
//   count     one 256-thread workgroup per row i: thread t takes the columns t, t + 256, ... (a
//             wavefront reads 64 consecutive 16-B cells, 1 KiB per load instruction); a cell is
//             reported when packets != 0 || weight != 0.  The row's reported cells go to
//             rowCells[i] (i64, the scan's input), its sums over all cells to sentP / sentW [i],
//             its {largest weight, lowest cell index} to rowPeakW / rowPeakCell [i] (a butterfly
//             with a symmetric tie rule, the waves merged in a few bytes of LDS); the column sums
//             are u64 atomics into recvP / recvW [j] for reported cells only (a cell that is not
//             reported adds zero), the totals one atomic per workgroup and counter;
//   scan      trace_exclusive_scan over the M + 1 row counts;
//   fill      a row with nothing to report, or one starting at or past cap, returns at once;
//             otherwise per 256-column step a wave ballot of "reported", the wave popcounts
//             through LDS, rank = row offset + earlier steps + earlier waves + prefix popcount:
//             records in (row, column) order with no sort and no atomic, 32 B each as two 16-B
//             stores; a record at or past cap is not written.
//
// Byte model.  feed: 8 B of columns, the weight (4 B payload, 8 B host weight or none) and 1 B of
// `delivered` per packet, plus two atomics on one 16-B cell; count: 16 M^2 B; fill: 16 B per cell
// of the rows it walks, plus 32 B per record written.
//
// Sums are u64 and wrap: any order of the atomics, any split of the packets into feeds, gives the
// same cells.  Every index is bounded before it is used: a column by A, a matrix index by M, a
// record by cap.
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

static_assert(sizeof(MatCell) == 16, "MatCell is one 16-B load");
static_assert(sizeof(MatFlowRec) == 32, "MatFlowRec is two 16-B stores");

__device__ __forceinline__ int64_t gtid() {
    return (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
}
__device__ __forceinline__ int64_t gstride() { return (int64_t)gridDim.x * blockDim.x; }
unsigned grid_for(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kTB - 1) / kTB, 65536));
}

__device__ __forceinline__ MatCell cell_load(const MatCell* __restrict__ c, size_t k) {
    const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(c + k);
    return MatCell{x.x, x.y};
}
__device__ __forceinline__ bool reported(const MatCell& c) { return (c.packets | c.weight) != 0; }

// One packet per thread and round.  W: the weight's type (u32 payload of a packet batch, u64 of a
// host feed).  cnt: the cumulative counters, then (at MX_COUNT) those of this feed.
template <class W>
__global__ void __launch_bounds__(kTB)
matrix_feed_kernel(int64_t n, const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                   const W* __restrict__ weight, const uint8_t* __restrict__ delivered,
                   const int32_t* __restrict__ colMap, int32_t A, MatCell* __restrict__ cells,
                   int32_t M, u64* __restrict__ cnt) {
    u64 fed = 0, skipped = 0, bad = 0;
    for (int64_t k = gtid(); k < n; k += gstride()) {
        if (delivered && __builtin_nontemporal_load(delivered + k) == 0) {
            skipped++;
            continue;
        }
        const uint32_t s = (uint32_t)__builtin_nontemporal_load(src + k);
        const uint32_t d = (uint32_t)__builtin_nontemporal_load(dst + k);
        if (s >= (uint32_t)A || d >= (uint32_t)A) {  // nothing is read through it
            bad++;
            continue;
        }
        const uint32_t i = (uint32_t)colMap[s], j = (uint32_t)colMap[d];
        if (i >= (uint32_t)M || j >= (uint32_t)M) {  // (the map covers every column)
            bad++;
            continue;
        }
        const u64 w = weight ? (u64)__builtin_nontemporal_load(weight + k) : 1ull;
        MatCell* c = cells + ((size_t)i * (size_t)M + j);  // adjacent words: one line
        atomicAdd(&c->packets, 1ull);
        if (w) atomicAdd(&c->weight, w);
        fed++;
    }
    // every lane reaches this point: one atomic per wavefront and counter
    const u64 v[MX_COUNT] = {wave_sum_u64(fed), wave_sum_u64(skipped), wave_sum_u64(bad)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < MX_COUNT; i++)
            if (v[i]) {
                atomicAdd(&cnt[i], v[i]);
                atomicAdd(&cnt[MX_COUNT + i], v[i]);
            }
    }
}

__global__ void __launch_bounds__(kTB)
matrix_relayout_kernel(const MatCell* __restrict__ old, int32_t M0, const int32_t* __restrict__ map,
                       MatCell* __restrict__ cells, int32_t M1) {
    const int64_t n = (int64_t)M0 * M0;
    for (int64_t k = gtid(); k < n; k += gstride()) {
        const int32_t i = (int32_t)(k / M0), j = (int32_t)(k - (int64_t)i * M0);
        const uint32_t a = (uint32_t)map[i], b = (uint32_t)map[j];
        if (a >= (uint32_t)M1 || b >= (uint32_t)M1) continue;  // (the map stays inside the new one)
        const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(old + k);
        *reinterpret_cast<ulonglong2*>(cells + ((size_t)a * (size_t)M1 + b)) = x;
    }
}

__global__ void __launch_bounds__(kTB)
matrix_add_kernel(MatCell* __restrict__ cells, const MatCell* __restrict__ add, int64_t n) {
    for (int64_t k = gtid(); k < n; k += gstride()) {
        const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(cells + k);
        const ulonglong2 y = *reinterpret_cast<const ulonglong2*>(add + k);
        *reinterpret_cast<ulonglong2*>(cells + k) = make_ulonglong2(x.x + y.x, x.y + y.y);
    }
}

__global__ void __launch_bounds__(kTB)
matrix_count_kernel(const MatCell* __restrict__ cells, int32_t M, MatCount o) {
    __shared__ u64 s_sum[kNW][6];  // cells, packets, weight, self cells, self packets, self weight
    __shared__ u64 s_peak[kNW];
    __shared__ int64_t s_cell[kNW];
    const int64_t i = blockIdx.x;  // grid = M
    const size_t base = (size_t)i * (size_t)M;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    u64 nrep = 0, p = 0, w = 0, sc = 0, sp = 0, sw = 0;
    u64 peak = 0;
    int64_t cell = -1;
    for (int32_t j = (int32_t)threadIdx.x; j < M; j += kTB) {
        const MatCell c = cell_load(cells, base + (size_t)j);
        if (!reported(c)) continue;  // (a cell that is not reported adds zero to every sum)
        nrep++;
        p += c.packets;
        w += c.weight;
        if (j == (int32_t)i) {
            sc = 1;
            sp = c.packets;
            sw = c.weight;
        }
        atomicAdd(&o.recvP[j], c.packets);
        if (c.weight) atomicAdd(&o.recvW[j], c.weight);
        o.colActive[j] = 1u;  // (every writer stores the same word)
        const int64_t k = (int64_t)base + j;
        if (worse_rise(c.weight, k, peak, cell)) {
            peak = c.weight;
            cell = k;
        }
    }
    const u64 v[6] = {wave_sum_u64(nrep), wave_sum_u64(p),  wave_sum_u64(w),
                      wave_sum_u64(sc),   wave_sum_u64(sp), wave_sum_u64(sw)};
    wave_worst_rise(peak, cell);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) s_sum[wid][k] = v[k];
        s_peak[wid] = peak;
        s_cell[wid] = cell;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t[6] = {0, 0, 0, 0, 0, 0};
        for (int wv = 0; wv < kNW; wv++) {
#pragma unroll
            for (int k = 0; k < 6; k++) t[k] += s_sum[wv][k];
            if (wv > 0 && worse_rise(s_peak[wv], s_cell[wv], peak, cell)) {
                peak = s_peak[wv];
                cell = s_cell[wv];
            }
        }
        o.rowCells[i] = (int64_t)t[0];
        o.sentP[i] = t[1];
        o.sentW[i] = t[2];
        o.rowPeakW[i] = cell >= 0 ? peak : 0ull;
        o.rowPeakCell[i] = cell;
        if (t[0]) {
            atomicAdd(&o.tot[MT_CELLS], t[0]);
            atomicAdd(&o.tot[MT_ACTIVE_SRC], 1ull);
        }
        if (t[1]) atomicAdd(&o.tot[MT_PACKETS], t[1]);
        if (t[2]) atomicAdd(&o.tot[MT_WEIGHT], t[2]);
        if (t[3]) atomicAdd(&o.tot[MT_SELF_CELLS], t[3]);
        if (t[4]) atomicAdd(&o.tot[MT_SELF_PACKETS], t[4]);
        if (t[5]) atomicAdd(&o.tot[MT_SELF_WEIGHT], t[5]);
    }
}

__global__ void __launch_bounds__(kTB)
matrix_fill_kernel(const MatCell* __restrict__ cells, int32_t M, const int32_t* __restrict__ mv,
                   const int64_t* __restrict__ rowCells, const int64_t* __restrict__ rowOff,
                   MatFlowRec* __restrict__ out, int64_t cap) {
    __shared__ uint32_t s_wave[kNW];
    const int64_t i = blockIdx.x;  // grid = M
    // (both conditions are the same for every thread of the workgroup)
    if (rowCells[i] == 0) return;
    int64_t pos = rowOff[i];
    if (pos >= cap) return;
    const size_t base = (size_t)i * (size_t)M;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int32_t sv = mv[i];
    for (int32_t j0 = 0; j0 < M; j0 += kTB) {
        const int32_t j = j0 + (int32_t)threadIdx.x;
        MatCell c{0ull, 0ull};
        if (j < M) c = cell_load(cells, base + (size_t)j);
        const bool rep = reported(c);
        const u64 m = __ballot(rep);
        if (lane == 0) s_wave[wid] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int wv = 0; wv < kNW; wv++) {
            const uint32_t n = s_wave[wv];
            before += wv < wid ? n : 0u;
            all += n;
        }
        if (rep) {
            const int64_t r = pos + (int64_t)before + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
            if (r < cap) {
                int4* q = reinterpret_cast<int4*>(out + r);
                q[0] = make_int4(sv, mv[j], (int32_t)i, j);
                *reinterpret_cast<ulonglong2*>(q + 1) = make_ulonglong2(c.packets, c.weight);
            }
        }
        pos += (int64_t)all;
        if (pos >= cap) return;  // (uniform: pos is the same in every thread)
        __syncthreads();         // s_wave is rewritten by the next step
    }
}

template <class W>
hipError_t feed(int64_t n, const int32_t* src, const int32_t* dst, const W* weight,
                const uint8_t* delivered, const int32_t* colMap, int32_t A, MatCell* cells,
                int32_t M, unsigned long long* cnt, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    // (A == 0: every column is outside [0, A), the packets are counted and nothing is read)
    if (!src || !dst || !cnt || !colMap || !cells || A < 0 || M < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL((matrix_feed_kernel<W>), dim3(grid_for(n)), dim3(kTB), 0, stream, n, src,
                       dst, weight, delivered, colMap, A, cells, M, cnt);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_matrix_feed(int64_t n, const int32_t* src, const int32_t* dst,
                              const uint32_t* payload, const uint8_t* delivered,
                              const int32_t* colMap, int32_t A, MatCell* cells, int32_t M,
                              unsigned long long* cnt, hipStream_t stream) {
    return feed<uint32_t>(n, src, dst, payload, delivered, colMap, A, cells, M, cnt, stream);
}

hipError_t launch_matrix_feed_u64(int64_t n, const int32_t* src, const int32_t* dst,
                                  const unsigned long long* weight, const uint8_t* delivered,
                                  const int32_t* colMap, int32_t A, MatCell* cells, int32_t M,
                                  unsigned long long* cnt, hipStream_t stream) {
    return feed<unsigned long long>(n, src, dst, weight, delivered, colMap, A, cells, M, cnt,
                                    stream);
}

hipError_t launch_matrix_relayout(const MatCell* old, int32_t M0, const int32_t* map,
                                  MatCell* cells, int32_t M1, hipStream_t stream) {
    if (M1 <= 0) return hipSuccess;
    if (!cells || M0 < 0 || M0 > M1 || (M0 > 0 && (!old || !map))) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(cells, 0, sizeof(MatCell) * (size_t)M1 * (size_t)M1, stream);
    if (e != hipSuccess || M0 == 0) return e;
    hipLaunchKernelGGL(matrix_relayout_kernel, dim3(grid_for((int64_t)M0 * M0)), dim3(kTB), 0,
                       stream, old, M0, map, cells, M1);
    return hipGetLastError();
}

hipError_t launch_matrix_add(MatCell* cells, const MatCell* add, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (!cells || !add) return hipErrorInvalidValue;
    hipLaunchKernelGGL(matrix_add_kernel, dim3(grid_for(n)), dim3(kTB), 0, stream, cells, add, n);
    return hipGetLastError();
}

hipError_t launch_matrix_count(const MatCell* cells, int32_t M, const MatCount& o,
                               hipStream_t stream) {
    if (M <= 0) return hipSuccess;
    if (!cells || !o.rowCells || !o.sentP || !o.sentW || !o.recvP || !o.recvW || !o.colActive ||
        !o.rowPeakW || !o.rowPeakCell || !o.tot)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(matrix_count_kernel, dim3((unsigned)M), dim3(kTB), 0, stream, cells, M, o);
    return hipGetLastError();
}

hipError_t launch_matrix_fill(const MatCell* cells, int32_t M, const int32_t* mv,
                              const int64_t* rowCells, const int64_t* rowOff, MatFlowRec* out,
                              int64_t cap, hipStream_t stream) {
    if (M <= 0 || cap <= 0) return hipSuccess;
    if (!cells || !mv || !rowCells || !rowOff || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(matrix_fill_kernel, dim3((unsigned)M), dim3(kTB), 0, stream, cells, M, mv,
                       rowCells, rowOff, out, cap);
    return hipGetLastError();
}

}  // namespace shdtopo
