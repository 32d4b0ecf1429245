// topo_shift.hip -- load shift for gfx950: where the load of a set of flows differs between two
// link loads that stay on the device.
//
// shdtopo_load_shift (include/shd_topology_abi.h) accumulates the flows on two topologies and
// compares the results entry by entry in the root topology's numbering: entry x in [0, 2 R + V) is
// the forward half of root edge x (x < R), the reverse half of root edge x - R (x < 2 R) or vertex
// x - 2 R.  A side's own id of a root edge is computed, not read from a map: the side carries the
// ascending list of the root ids it lacks (ShiftSide.gaps; a handful after a link failure, none
// for a root topology) and root edge r is its edge r - (the gaps below r), by a binary search of
// that list.  The tiling is topo_impact.hip's: 256 threads per workgroup, workgroup blk owns the
// entries [blk 256 U, (blk + 1) 256 U), thread t takes base + j 256 + t for j < U, so a
// (wavefront, j) is 64 consecutive entries and its __ballot is word x / 64 of a bitmap of the
// changed entries.
//
//   count   ids first, then all 2 U loads before any is used: the ids ascend with the lanes, so a
//           wavefront's gather is a run of consecutive u64 with at most ngaps breaks.  Lane 0
//           writes the ballot word of each (wavefront, j).  The fifteen counts by kind come from
//           popcounts of ballots; the eight weighted sums are reduced by wave butterflies in a
//           wavefront that has a change, meet in LDS and leave as one u64 atomic per non-zero
//           total and workgroup.  Every sum wraps: any order gives the same result.  The tile's
//           four {largest value, lowest entry} pairs -- gain, loss, peak before, peak after -- are
//           merged by topo_paircmp.h's rule on u64;
//   reduce  one workgroup merges the tiles' pairs by the same rule into the call's four;
//   scan    trace_exclusive_scan over the tiles' changed counts: each tile's first record;
//   fill    the same tiling.  Every thread reads its tile's 4 U words: a changed lane's rank is the
//           tile's offset + the popcounts of the earlier words + the popcount below the lane -- no
//           atomic, no sort, no barrier.  A word that is zero, or starts at or past cap, gathers
//           nothing; only changed lanes load again and write their 32-B record (two 16-B stores).
//
// No kernel stores outside words [tiles x 4 U], tileChanged [tiles], tileVal / tileIdx [tiles x
// SP_COUNT], tot [SH_COUNT], pairVal / pairIdx [SP_COUNT], gathered [kImpactShards x
// kImpactShardStride] and out [min(total, cap)]: every index is bounded by x < 2 R + V (a word's
// bits are set for entries below it only) or pos < cap.  Every load index is bounded likewise: a
// side's id is below its E because its gaps are R - E distinct ids of [0, R) (checked on the host).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "topo_dev_common.h"
#include "topo_paircmp.h"

namespace shdtopo {

namespace {

using namespace dev;
using u64 = unsigned long long;

#ifndef SHD_SHIFT_U
#define SHD_SHIFT_U 2
#endif
constexpr int kTB = 256;
constexpr int kNW = kTB / 64;
constexpr int kU = SHD_SHIFT_U;   // entries per thread: 2 kU loads in flight
constexpr int kWords = kNW * kU;  // ballot words per tile

static_assert(sizeof(ShiftRec) == 32, "ShiftRec is two 16-B stores");
static_assert(kU >= 1 && kU <= 8, "entries per thread");
static_assert(SH_COUNT <= kTB && SP_COUNT == 4, "one thread per total; four pairs");

// LDS of the count pass (u64 words): the totals, then the waves' pair values and entries
constexpr int kLdsTot = 0, kLdsVal = SH_COUNT, kLdsIdx = kLdsVal + SP_COUNT * kNW,
              kLdsWords = kLdsIdx + SP_COUNT * kNW;

// the side's id of root edge r; -1: it lacks the edge
__device__ __forceinline__ int32_t side_id(const ShiftSide& s, int32_t r) {
    int lo = 0, hi = s.ngaps;  // the number of gaps below r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s.gaps[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    if (lo < s.ngaps && s.gaps[lo] == r) return -1;
    return r - lo;
}

struct Entry {
    int32_t kind, id, idA, idB;
};
// entry x < 2 R + V
__device__ __forceinline__ Entry entry_of(const ShiftIn& in, int64_t x) {
    Entry e;
    if (x >= 2 * in.R) {
        e.kind = 2;
        e.id = e.idA = e.idB = (int32_t)(x - 2 * in.R);
    } else {
        e.kind = x >= in.R ? 1 : 0;
        e.id = (int32_t)(e.kind ? x - in.R : x);
        e.idA = side_id(in.a, e.id);
        e.idB = side_id(in.b, e.id);
    }
    return e;
}
// where the side keeps the entry's load (nullptr: it lacks the edge, the load is 0)
__device__ __forceinline__ const u64* load_of(const ShiftSide& s, int32_t kind, int32_t id) {
    if (id < 0) return nullptr;
    return kind == 2 ? s.vload + id : s.eload + (kind ? s.E : 0) + id;
}

__global__ __launch_bounds__(kTB) void shift_count_kernel(ShiftIn in, ShiftOut o) {
    __shared__ u64 lds[kLdsWords];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int i = (int)threadIdx.x; i < SH_COUNT; i += kTB) lds[kLdsTot + i] = 0ull;
    __syncthreads();

    const int64_t X = 2 * in.R + in.V;
    const int64_t base = (int64_t)blockIdx.x * (kTB * kU) + threadIdx.x;
    Entry en[kU];
    const u64 *pa[kU], *pb[kU];
#pragma unroll
    for (int j = 0; j < kU; j++) {
        const int64_t x = base + (int64_t)j * kTB;
        en[j] = Entry{0, 0, -1, -1};
        pa[j] = pb[j] = nullptr;
        if (x < X) {
            en[j] = entry_of(in, x);
            pa[j] = load_of(in.a, en[j].kind, en[j].idA);
            pb[j] = load_of(in.b, en[j].kind, en[j].idB);
        }
    }
    u64 bef[kU], aft[kU];
#pragma unroll
    for (int j = 0; j < kU; j++) {
        bef[j] = pa[j] ? *pa[j] : 0ull;
        aft[j] = pb[j] ? *pb[j] : 0ull;
    }

    // wave-uniform counts (from ballots) and per-lane weighted sums
    uint32_t nChanged = 0, cnt[15] = {};
    u64 gw[3] = {0, 0, 0}, lw[3] = {0, 0, 0}, disp = 0, app = 0;
    u64 val[SP_COUNT] = {0, 0, 0, 0};
    int64_t idx[SP_COUNT] = {-1, -1, -1, -1};
#pragma unroll
    for (int j = 0; j < kU; j++) {
        const int64_t x = base + (int64_t)j * kTB;
        const bool in_range = x < X;
        const int32_t kind = en[j].kind;
        const u64 b = bef[j], a = aft[j];
        const bool ch = in_range && b != a;
        const u64 m = __ballot(ch);
        if (lane == 0) o.words[(int64_t)blockIdx.x * kWords + j * kNW + wid] = m;
        // a thread's entries ascend: the first to reach a maximum stays
        if (in_range && kind < 2) {
            if (b > val[SP_PEAK_BEFORE]) {
                val[SP_PEAK_BEFORE] = b;
                idx[SP_PEAK_BEFORE] = x;
            }
            if (a > val[SP_PEAK_AFTER]) {
                val[SP_PEAK_AFTER] = a;
                idx[SP_PEAK_AFTER] = x;
            }
        }
        if (m == 0ull) continue;  // (the same in every lane of the wavefront)
        nChanged += (uint32_t)__popcll(m);
        const u64 mG = __ballot(ch && a > b), mN = __ballot(ch && b == 0ull),
                  mA = __ballot(ch && a == 0ull);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const u64 mk = __ballot(in_range && kind == k);
            cnt[SH_CHANGED + k] += (uint32_t)__popcll(m & mk);
            cnt[SH_GAINED + k] += (uint32_t)__popcll(mG & mk);
            cnt[SH_LOST + k] += (uint32_t)__popcll(m & ~mG & mk);
            cnt[SH_NEW + k] += (uint32_t)__popcll(mN & mk);
            cnt[SH_ABANDONED + k] += (uint32_t)__popcll(mA & mk);
        }
        if (!ch) continue;
        const bool up = a > b;
        const u64 d = up ? a - b : b - a;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            gw[k] += up && kind == k ? d : 0ull;
            lw[k] += !up && kind == k ? d : 0ull;
        }
        // (a half its side lacks has load 0 there: only a changed entry adds to these)
        if (kind < 2 && en[j].idB < 0) disp += b;
        if (kind < 2 && en[j].idA < 0) app += a;
        // (d > 0; static indices: the pairs stay in registers)
        if (up && d > val[SP_GAIN]) {
            val[SP_GAIN] = d;
            idx[SP_GAIN] = x;
        }
        if (!up && d > val[SP_LOSS]) {
            val[SP_LOSS] = d;
            idx[SP_LOSS] = x;
        }
    }

    // the wavefront's sums and pairs; those of the changed entries only where it has one
    if (nChanged) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            gw[k] = wave_sum_u64(gw[k]);
            lw[k] = wave_sum_u64(lw[k]);
        }
        disp = wave_sum_u64(disp);
        app = wave_sum_u64(app);
        wave_worst_rise(val[SP_GAIN], idx[SP_GAIN]);
        wave_worst_rise(val[SP_LOSS], idx[SP_LOSS]);
    }
    wave_worst_rise(val[SP_PEAK_BEFORE], idx[SP_PEAK_BEFORE]);
    wave_worst_rise(val[SP_PEAK_AFTER], idx[SP_PEAK_AFTER]);
    if (lane == 0) {
        auto add = [&](int i, u64 v) {
            if (v) atomicAdd(&lds[kLdsTot + i], v);
        };
        if (nChanged) {
#pragma unroll
            for (int i = 0; i < 15; i++) add(i, cnt[i]);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                add(SH_GAINED_W + k, gw[k]);
                add(SH_LOST_W + k, lw[k]);
            }
            add(SH_DISPLACED, disp);
            add(SH_APPEARED, app);
        }
#pragma unroll
        for (int p = 0; p < SP_COUNT; p++) {
            lds[kLdsVal + p * kNW + wid] = val[p];
            lds[kLdsIdx + p * kNW + wid] = (u64)idx[p];
        }
    }
    __syncthreads();
    if (threadIdx.x < SH_COUNT && lds[kLdsTot + threadIdx.x])
        atomicAdd(&o.tot[threadIdx.x], lds[kLdsTot + threadIdx.x]);
    if (threadIdx.x < SP_COUNT) {
        const int p = (int)threadIdx.x;
        u64 v = lds[kLdsVal + p * kNW];
        int64_t c = (int64_t)lds[kLdsIdx + p * kNW];
        for (int q = 1; q < kNW; q++) {
            const u64 r = lds[kLdsVal + p * kNW + q];
            const int64_t ci = (int64_t)lds[kLdsIdx + p * kNW + q];
            if (worse_rise(r, ci, v, c)) {
                v = r;
                c = ci;
            }
        }
        o.tileVal[(int64_t)blockIdx.x * SP_COUNT + p] = c >= 0 ? v : 0ull;
        o.tileIdx[(int64_t)blockIdx.x * SP_COUNT + p] = c;
    }
    if (threadIdx.x == 0) {
        u64 n = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) n += lds[kLdsTot + SH_CHANGED + k];
        o.tileChanged[blockIdx.x] = (int64_t)n;
    }
}

// one workgroup: wavefront p merges pair p of every tile
__global__ __launch_bounds__(kTB) void shift_reduce_kernel(int64_t tiles,
                                                           const u64* __restrict__ tileVal,
                                                           const int64_t* __restrict__ tileIdx,
                                                           u64* __restrict__ pairVal,
                                                           int64_t* __restrict__ pairIdx) {
    const int lane = threadIdx.x & 63, p = threadIdx.x >> 6;  // (kNW == SP_COUNT)
    u64 v = 0;
    int64_t c = -1;
    for (int64_t k = lane; k < tiles; k += 64) {
        const u64 r = tileVal[k * SP_COUNT + p];
        const int64_t ci = tileIdx[k * SP_COUNT + p];
        if (worse_rise(r, ci, v, c)) {
            v = r;
            c = ci;
        }
    }
    wave_worst_rise(v, c);
    if (lane == 0) {
        pairVal[p] = c >= 0 ? v : 0ull;
        pairIdx[p] = c;
    }
}
static_assert(kNW == SP_COUNT, "shift_reduce_kernel: one wavefront per pair");

__global__ __launch_bounds__(kTB) void shift_fill_kernel(ShiftIn in, const u64* __restrict__ words,
                                                         const int64_t* __restrict__ tileChanged,
                                                         const int64_t* __restrict__ tileOff,
                                                         ShiftRec* __restrict__ out, int64_t cap,
                                                         u64* gathered) {
    // (both conditions are the same for every thread of the workgroup)
    if (tileChanged[blockIdx.x] == 0) return;
    int64_t run = tileOff[blockIdx.x];
    if (run >= cap) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const u64* bw = words + (int64_t)blockIdx.x * kWords;
    // this wavefront's words and the rank of their first changed entry: words in entry order
    u64 mine[kU];
    int64_t first[kU];
#pragma unroll
    for (int q = 0; q < kWords; q++) {
        const u64 m = bw[q];
        if (q % kNW == wid) {
            mine[q / kNW] = m;
            first[q / kNW] = run;
        }
        run += (int64_t)__popcll(m);
    }
    const int64_t base = (int64_t)blockIdx.x * (kTB * kU) + threadIdx.x;
    uint32_t ng = 0;
#pragma unroll
    for (int j = 0; j < kU; j++) {
        const u64 m = mine[j];
        if (m == 0ull || first[j] >= cap) continue;  // (wave-uniform) nothing to gather for
        ng++;
        if (!((m >> lane) & 1ull)) continue;
        const int64_t p = first[j] + (int64_t)__popcll(m & ((1ull << lane) - 1ull));
        if (p >= cap) continue;
        const int64_t x = base + (int64_t)j * kTB;  // (< 2 R + V: the bit is set)
        const Entry e = entry_of(in, x);
        const u64* pa = load_of(in.a, e.kind, e.idA);
        const u64* pb = load_of(in.b, e.kind, e.idB);
        ShiftRec r;
        r.kind = e.kind;
        r.id = e.id;
        r.idA = e.idA;
        r.idB = e.idB;
        r.before = pa ? *pa : 0ull;
        r.after = pb ? *pb : 0ull;
        out[p] = r;
    }
    if (lane == 0 && ng)
        atomicAdd(&gathered[(blockIdx.x % kImpactShards) * kImpactShardStride], (u64)ng);
}

int64_t tiles_of(int64_t n) { return (n + kTB * kU - 1) / (kTB * kU); }

bool side_ok(const ShiftSide& s, int64_t R, int64_t V) {
    if (s.E < 0 || s.ngaps < 0 || s.E + s.ngaps != R || (s.ngaps > 0 && !s.gaps)) return false;
    return (s.E == 0 || s.eload) && (V == 0 || s.vload);
}
bool in_ok(const ShiftIn& in) {
    return in.R >= 0 && in.V >= 0 && in.R <= INT32_MAX && in.V <= INT32_MAX &&
           side_ok(in.a, in.R, in.V) && side_ok(in.b, in.R, in.V);
}

}  // namespace

int64_t shift_tile_entries() { return (int64_t)kTB * kU; }

hipError_t launch_shift_count(const ShiftIn& in, const ShiftOut& o, hipStream_t stream) {
    const int64_t X = 2 * in.R + in.V;
    if (X <= 0) return hipSuccess;
    const int64_t tiles = tiles_of(X);
    if (!in_ok(in) || tiles > INT32_MAX) return hipErrorInvalidValue;
    if (!o.words || !o.tileChanged || !o.tileVal || !o.tileIdx || !o.tot)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(shift_count_kernel, dim3((unsigned)tiles), dim3(kTB), 0, stream, in, o);
    return hipGetLastError();
}

hipError_t launch_shift_reduce(int64_t tiles, const unsigned long long* tileVal,
                               const int64_t* tileIdx, unsigned long long* pairVal,
                               int64_t* pairIdx, hipStream_t stream) {
    if (tiles < 0 || !tileVal || !tileIdx || !pairVal || !pairIdx) return hipErrorInvalidValue;
    hipLaunchKernelGGL(shift_reduce_kernel, dim3(1), dim3(kTB), 0, stream, tiles, tileVal, tileIdx,
                       pairVal, pairIdx);
    return hipGetLastError();
}

hipError_t launch_shift_fill(const ShiftIn& in, const unsigned long long* words,
                             const int64_t* tileChanged, const int64_t* tileOff, ShiftRec* out,
                             int64_t cap, unsigned long long* gathered, hipStream_t stream) {
    const int64_t X = 2 * in.R + in.V;
    if (X <= 0 || cap <= 0) return hipSuccess;
    const int64_t tiles = tiles_of(X);
    if (!in_ok(in) || tiles > INT32_MAX) return hipErrorInvalidValue;
    if (!words || !tileChanged || !tileOff || !out || !gathered) return hipErrorInvalidValue;
    hipLaunchKernelGGL(shift_fill_kernel, dim3((unsigned)tiles), dim3(kTB), 0, stream, in, words,
                       tileChanged, tileOff, out, cap, gathered);
    return hipGetLastError();
}

}  // namespace shdtopo
