// mc_launch_shape.hpp -- every rule that decides the SHAPE of a launch: how many workgroups a call gets, which kernel
// family prices a basket of n assets, how many pieces the launch-geometry kernels cut a thread's stream into.  Host-only
// code, included by mc_api.hip alone.  It lives in a file of its own because the committed PMC profiles
// (profiles/pmc_traffic.json: instruction counts, waves, HBM bytes per launch) describe launches of exactly this shape:
// bench.py and tools/summarize_pmc.py hash this file together with the device code object, and a change here marks the
// counts stale (tests/test_host_logic.py::test_pmc_stamp_covers_the_launch).
#pragma once
#include <stdint.h>

#include <cstdlib>
#include <vector>

#include "../../include/mc_mi355x.h"
#include "mc_grid.hpp"   // GROUP, GRID_SEG_ALIGN

namespace mc {

static constexpr int MAX_SEGMENTS = 8;   // per call: segments of <= 2^31 units, same high word
static constexpr int MAX_GRID_SCALE = 6; // the heaviest kernels launch up to this many times the context's `blocks` (grid_for)

static int env_int(const char *name, int fallback, int lo, int hi)
{
    const char *e = getenv(name);
    const int v = e ? atoi(e) : fallback;
    return v < lo ? lo : (v > hi ? hi : v);
}

// Workgroups of a launch over n_units units: one lane per unit until the grid reaches `scale` x the context's `blocks`
// (default 8 per CU = 2048), grid-stride beyond.  `scale` (halves: 2 = 1x) grows with the weight of a unit.  All workgroups
// of a launch do equal work, but they do not finish together (CUs and XCDs run at slightly different rates, and a kernel
// whose registers admit only 4-6 workgroups per CU runs the grid in several rounds): more, smaller workgroups even that
// out.  Measured at the BASELINE sizes, grids of 4 ... 64 per CU interleaved in one process
// (tools/grid_sweep_all.py, profiles/r03_grid_sweep.log), kernel time against 8 per CU:
//     vanilla f32, basket f32 <= 12 assets    8 per CU is the optimum (16: +1...3 %)
//     vanilla f64, CVA f64 / f32             12 per CU: -1.0 / -1.9 / -1.7 %  (flat beyond; vanilla worse from 32)
//     tiled basket f32 (13..32 assets)       24 per CU: -1.8 %
//     tiled basket f64 (9..32 assets)        48 per CU: -4.2 %  (C4's kernel: still improving slowly at 64)
// The XORWOW policy keeps 1x (its per-lane states are sized by `blocks`), so do the secondary (Greeks) kernels.
static int grid_for(int blocks, uint32_t n_units, int scale_halves = 2)
{
    const uint64_t need = ((uint64_t)n_units + GROUP - 1) / GROUP, cap = (uint64_t)blocks * (uint64_t)scale_halves / 2;
    return (int)(need < cap ? (need ? need : 1) : cap);
}
constexpr int GRID_SCALE_VANILLA_F64 = 3, GRID_SCALE_CVA = 3, GRID_SCALE_TILED_F32 = 6, GRID_SCALE_TILED_F64 = 2 * MAX_GRID_SCALE;

// Vanilla launches whose units are cheap (4 or 2 paths each): a SMALL call is dominated by what grows with the grid --
// dispatch, one pair and one ticket per workgroup, the last arriver's sum over the pairs -- not by the simulation.  So a
// lane gets at least 4 units before the grid grows beyond one workgroup per CU: the 8 x 131 072-path call (the reference
// drivers' smallest size) runs 256 workgroups instead of 1024 (kernel 7.9 instead of 8.8 us in fp32, 10.1 instead of 12.0 in fp64:
// profiles/r02_call_latency.log); from 2.1e6 units (8.4e6 fp32 paths) on the grid is the context's `blocks` as before (16 units per lane
// measured no better at 1e7 paths).  MC_VANILLA_UNITS_PER_LANE=1 restores
// one unit per lane.
static int vanilla_units_per_lane()
{
    static const int v = [] {
        const char *e = getenv("MC_VANILLA_UNITS_PER_LANE");
        const int x = e ? atoi(e) : 4;
        return x < 1 ? 1 : (x > 1024 ? 1024 : x);
    }();
    return v;
}
static int grid_for_vanilla(int blocks, int compute_units, uint32_t n_units, int scale_halves)
{
    const int full = grid_for(blocks, n_units, scale_halves);
    const uint64_t per = (uint64_t)GROUP * (uint64_t)vanilla_units_per_lane();
    uint64_t want = ((uint64_t)n_units + per - 1) / per;
    const uint64_t floor_wgs = (uint64_t)(compute_units > 0 ? compute_units : 256);
    if (want < floor_wgs)
        want = floor_wgs;
    return (int)(want < (uint64_t)full ? want : (uint64_t)full);
}

// fp32 vanilla, Philox: which units of a segment run BLOCKED (mc_kernels.hpp: vanilla_f32_blocked_kernel -- a lane takes whole
// 8-aligned blocks of 8 units, 481 VALU instructions per block against 500 for 8 unit-strided trips).  A block is 8 x coarser
// than a unit, so the rule is written in unit-trips of the whole grid (stride = lanes of the launch; a SWEEP = 8 stride units):
//   * the units below the first multiple of 8 (`head`, at most 7) are unit-strided;
//   * every full sweep is blocked;
//   * what is left after the last full sweep, R units, costs ceil(R / stride) trips unit-strided and 8 as one more, PARTIAL,
//     sweep (lanes below the remaining block count take one block, the others wait): blocked only if R > 7.5 stride, else
//     unit-strided in the same launch, from the last lane down.  So a call that ends just past a sweep leaves no lane behind
//     an 8-unit straggler.  The 1e8-path call on the default grid (25 000 000 units, 2048 x 256 lanes) is 5 full sweeps +
//     503 560 blocks (96 % of the lanes) in the sixth: every unit blocked;
//   * a segment of less than vanilla_blocked_min_sweeps() = 1 full sweep is not blocked at all and runs vanilla_f32_kernel,
//     the unit-strided loop alone, exactly as before.
// Measured against the build before, alternating in one process (tools/c/ab_libs van32, event-bracketed launches on the
// default grid, profiles/ab_vanilla_f32_blocked_sizes.log; a sweep is 16 777 216 paths):
//     1e4 ... 1.5e7 paths (below one sweep, the same kernel as before)   -1.1 ... +2.4 %: the run-to-run spread of these calls
//     1 sweep, 1 sweep + 64 units, 2 sweeps                              -3.4, -3.1 (-2.7 antithetic), -2.8 %
//     1.5, 3.5, 5.5 sweeps (4 unit-strided trips after the sweeps)       -0.7, -2.0, -1.9 %
//     1.9, 2.9 sweeps (7.2 unit-strided trips after the sweeps)          +0.4 ... +0.7, -1.0 %
//     3.95 sweeps, 1e8 paths (5.96 sweeps; a partial sweep)              -1.1, -2.1 % (1e8 -+ 8 units -1.9, -1.8; antithetic -1.9 %)
//   The first form -- ONE kernel that decided the split itself (three scalar divisions in its prologue) and took a partial
//   sweep from 7 strides on, also without a full sweep -- cost the small calls +4.1, +1.8, +1.1, +1.6, +0.9 % at 1e4, 1e5, 1e6,
//   4e6, 1e7 paths and +3.3 % at 1.5e7 (0.89 of a sweep, a partial sweep alone)
//   [profiles/ab_vanilla_f32_blocked_first_form.log]: hence a kernel of its own above the limit, the split as a kernel
//   argument, no blocks below one full sweep, and 7.5 strides before a partial sweep is taken.
// MC_VANILLA_BLOCKED_MIN_SWEEPS moves the limit for experiments (0 = block whatever has a block; a large value = never).
static uint32_t vanilla_blocked_min_sweeps()
{
    static const int v = env_int("MC_VANILLA_BLOCKED_MIN_SWEEPS", 1, 0, 1 << 30);
    return (uint32_t)v;
}
static VanillaBlocking vanilla_blocking(uint32_t unit_lo, uint32_t n_units, uint32_t stride)
{
    VanillaBlocking b = {0, 0, 0, 0, 0};
    const uint32_t head = (0u - unit_lo) & 7u;
    if (stride == 0 || n_units < head + 8u)
        return b;
    const uint32_t n_blocks = (n_units - head) >> 3, sweeps = n_blocks / stride;
    const uint64_t left_units = (uint64_t)(n_units - head) - 8ull * sweeps * stride;
    const uint32_t extra = 2ull * left_units > 15ull * stride ? n_blocks - sweeps * stride : 0u;
    if (sweeps < vanilla_blocked_min_sweeps() || sweeps + extra == 0)
        return b;
    b.head = head, b.sweeps = sweeps, b.extra = extra, b.blocked = 8u * (sweeps * stride + extra);
    b.rest_trips = (n_units - head - b.blocked) / stride;
    return b;
}

// Which kernel family prices a basket of n assets (measured on MI355X: tools/generic_basket_speed.py, runs
// alternated in one gpurun call):
//   n <= basket_static_max (fp32: 12, fp64: 8)
//                      constants as kernel arguments / LDS-staged (basket_f32_kernel, basket_kernel)
//   up to 32 assets    constants as scalar-loaded tiles, normals in registers (basket_tiled_f32_kernel,
//                      basket_tiled_kernel).  fp64 9..16, one kernel per size: +3 % at 9, +14...+20 % at 10..16 over
//                      the kernel-argument form; fp32 13, 14, 16 (15 runs the 16 kernel): +5...+8 %, below 12 the
//                      LDS-staged form wins; 17..32: one kernel per multiple of 4 on the zero-padded buffer,
//                      +19...+39 % over the generic kernel
//   33..64 assets      generic tiled kernel, normals in LDS (basket_dyn_kernel, basket_dyn_f32_kernel)
//   MC_BASKET_MFMA=1   fp64, 13..16 assets: the mat-vec as v_mfma_f64_16x16x4_f64 (basket_mfma_f64_kernel).  Off by
//                      default: 5-6 % slower than the tiled kernel, the f64 matrix instruction does not run beside
//                      the vector pipe on gfx950 (profiles/r02_mfma_basket.log)
// MC_BASKET_STATIC_MAX_F32 / _F64 and MC_BASKET_TILED_MIN (read once per process) move the limits for
// experiments and for the tests that compare the families.
template <class Real>
static int basket_static_max()
{
    static const int limit = sizeof(Real) == 4 ? env_int("MC_BASKET_STATIC_MAX_F32", 12, 0, MC_MAX_ASSETS)
                                               : env_int("MC_BASKET_STATIC_MAX_F64", 8, 0, MC_MAX_ASSETS);
    return limit;
}
static bool basket_mfma()
{
    static const int on = env_int("MC_BASKET_MFMA", 0, 0, 1);
    return on != 0;
}
static int basket_tiled_min()
{
    static const int limit = env_int("MC_BASKET_TILED_MIN", 9, 9, 1000);
    return limit;
}

// CVA: how a call of n paths over n_dates dates is cut between one lane per path (cva_kernel; the date walk serial, as in the
// reference) and the date-parallel form (2^log2_lanes adjacent lanes per path, CVA_DATES_CH dates per lane and round; mc_kernels.hpp).
//   main_paths   leading paths, one lane each
//   tail_paths   trailing paths, date-parallel (both > 0: one launch of cva_split_kernel; main_paths == 0: cva_dates_kernel)
// The one-lane-per-path kernel's time is a staircase in steps of one WAVE-TRIP = 64 lanes x 4 SIMDs x CUs paths (65 536 on
// MI355X): a launch pays for whole trips -- 1 250 000 paths (C5's shard of 8: 19.07 trips) cost what 1 310 720 do, 990.9 us against
// 944.8 for 19 trips -- and a wave alone on its SIMD needs ~85 us (fp64; ~49 us fp32) for a 256-date path whatever the call's size.
// Measured with tools/c/shard_clock and tools/cva_call_latency.py (profiles/r06_shard_clock_AD_fused_split.log,
// profiles/r06_cva_call_latency.log):
//   * a call of more than the small-call limit and at most 64 trips, on a grid of at least 64 dates, that ends in a partial trip
//     of at most 60 % hands that remainder to date-parallel workgroups of the same launch, with enough lanes per path to put
//     about two of their waves on every SIMD (1 250 000 paths x 256 dates: fp64 990.9 -> 953.0 us, fp32 -4 %; the gain
//     shrinks to nothing as the remainder approaches a full trip: 0.31 of a trip -21.6 us, 0.45 -15.2, 0.53 -8.0; beyond 64 trips
//     a trip is under 1.6 % of the call);
//   * a SMALL call runs date-parallel as a whole, with lanes for ~4 waves per SIMD.  What "small" is depends on how long a
//     lane's serial walk is (the one-lane kernel's second wave on a SIMD costs it a third of the first: 256 dates fp64 85 us for
//     one trip, 113 for two; fp32 49 and 59), in both precisions alike:
//         >= 64 dates: up to 7/4 trips (256 dates, kernel time in us, fp64: 4096 paths 83 -> 15, 65 536: 84 -> 68, 98 304: 113 -> 95,
//                                       114 688: 113 -> 108; 131 072 -- the reference driver's own call, dp/cvaOpt.cu:12-15 -- 113 -> 121,
//                                       worse; fp32: 4096 paths 49 -> 11, 65 536: 49 -> 35, 98 304: 58 -> 48, 114 688: 59 -> 53, 131 072: a tie)
//         <  64 dates: up to 3/4 trip  (25 dates, fp64: 16 384 paths 15.6 -> 11.6, 49 152: 16.2 -> 15.2; 65 536: 15.7 -> 17.2, worse;
//                                       fp32: 16 384 paths 11.3 -> 8.9, 49 152: 11.6 -> 11.1; 65 536: 11.7 -> 12.2, worse)
//     (the date-parallel form pays per-lane table rows and per-lane Philox counters: +6 % at 2 lanes, +11 % at 8, +19...22 % from
//     16 on at 1e6 fp64 paths);
//   * everything else keeps one lane per path.
// `forced_lanes`: 0 = this rule, 1 = one lane per path always, 2 ... 64 = the whole call date-parallel with that many lanes
// (mc_context_set_cva_date_lanes / MC_CVA_DATE_LANES; the tests sweep it).  A path cannot use more lanes than it has
// chunks of CVA_DATES_CH dates.
constexpr int CVA_DATES_CH = 8;
struct CvaPlan { uint64_t main_paths, tail_paths; int log2_lanes; };
static int cva_max_log2_lanes(int n_dates)
{
    int l = 0;
    while (l < 6 && (CVA_DATES_CH << l) < n_dates)
        ++l;
    return l;
}
static CvaPlan cva_plan(int forced_lanes, uint64_t n, int n_dates, int compute_units, bool dates_kernel_possible, size_t real_bytes)
{
    constexpr int tail_max_pct = 60, small_fill = 4, split_max_trips = 64, long_grid = 64;
    const int small_trips_x4 = n_dates >= long_grid ? 7 : 3;   // quarter trips, inclusive
    (void)real_bytes;
    const int max_l = cva_max_log2_lanes(n_dates);
    CvaPlan p = {n, 0, 0};
    if (!dates_kernel_possible || max_l == 0 || forced_lanes == 1 || n == 0)
        return p;
    const auto log2_ceil = [](uint64_t x) { int l = 0; while ((1ull << l) < x) ++l; return l; };
    if (forced_lanes >= 2) {
        int l = 0;
        while ((2 << l) <= forced_lanes) ++l;
        p.main_paths = 0, p.tail_paths = n, p.log2_lanes = l < max_l ? l : max_l;
        return p;
    }
    const uint64_t trip = 64ull * 4ull * (uint64_t)(compute_units > 0 ? compute_units : 256);
    if (4 * n <= (uint64_t)small_trips_x4 * trip) {   // small call: all of it date-parallel, ~small_fill waves per SIMD
        int l = log2_ceil(((uint64_t)small_fill * trip + n - 1) / n);
        l = l > max_l ? max_l : l;
        if (l > 0)
            p.main_paths = 0, p.tail_paths = n, p.log2_lanes = l;
        return p;
    }
    const uint64_t r = n % trip;
    if (r == 0 || 100 * r > (uint64_t)tail_max_pct * trip || n > (uint64_t)split_max_trips * trip || n_dates < long_grid)
        return p;
    int l = log2_ceil((2 * trip + r - 1) / r);
    l = l < 1 ? 1 : (l > max_l ? max_l : l);
    p.main_paths = n - r, p.tail_paths = r, p.log2_lanes = l;
    return p;
}

// Vanilla books (mc_vanilla_book_*, mc_kernels.hpp vanilla_book_*): the chunks of every entry.  An entry of paths [first, end) in
// units of `npb` paths gets, in unit order:
//   * a masked chunk of ONE unit for a partial first unit, and one for a partial last unit (the single call's edge launches): its
//     `masked` word has bit j set for each path j of the unit inside the entry's range;
//   * the whole units between them in chunks of max(book_chunk_min, units / BOOK_CHUNKS_MAX rounded up to whole 256-lane trips)
//     units -- at most ~BOOK_CHUNKS_MAX chunks however large the entry -- also cut at every multiple
//     of 2^32 units (a chunk's high counter word is wave-uniform).
// So the boundaries are a function of the entry's own (first, n), precision and estimator: what makes an entry's triple the same
// bits wherever it sits in a book.  Ticket words: an entry of c chunks draws on s = ceil(c / BOOK_SHARD_CHUNKS) shard words
// (chunk j on shard j % s, at most BOOK_SHARD_CHUNKS arrivals each) and, when s > 1, on a top word of its own (s arrivals), each word
// of such an entry on a 128-byte line of its own (TICKET_STRIDE, as arrive_and_finish's tickets): a large entry never serialises
// thousands of arrivals on one word or line (~11-13 ns each, MI355X_MICROARCH.md "fanin").
// Refused (the index of the first bad entry is reported): what the single call refuses -- n == 0, a range past 2^64, n > 2^52,
// more than MAX_SEGMENTS segments of whole units -- and a book of more than BOOK_MAX_CHUNKS chunks in all (the entry named is
// the one at which the count passes the limit; nothing is stored before that is known).
constexpr uint32_t BOOK_CHUNKS_MAX = 2048, BOOK_SHARD_CHUNKS = 64;
// a chunk of whole units is at least what a lane of the single 1e8-path call does on the default grid (fp32 48 units, fp64 16): a
// chunk pays scalar table loads, a workgroup reduction and a returning agent-scope atomic, which 6 units per lane did not amortise
// (profiles/book_speed.log: 8 x 1.25e7-path entries +58 % over one 1e8-path call in fp32 with chunks of 6 units per lane)
static uint64_t book_chunk_min(uint32_t npb) { return (npb == 4 ? 48ull : 16ull) * GROUP; }
constexpr uint64_t BOOK_MAX_CHUNKS = 1ull << 24;
struct BookRange { uint64_t first_path, n_paths; };
struct BookSpan { uint32_t chunk0, chunks, shards, counter0; };
enum BookRefusal { BOOK_OK, BOOK_EMPTY, BOOK_OVERFLOW, BOOK_TOO_MANY_PATHS, BOOK_TOO_MANY_SEGMENTS, BOOK_TOO_MANY_CHUNKS };
struct BookPlan {
    std::vector<BookChunk> chunks;
    std::vector<BookSpan> spans;   // per entry
    uint32_t counter_words = 0;
    int bad_entry = -1;            // the first refused entry
};
static uint64_t book_chunk_units(uint64_t units, uint32_t npb)
{
    uint64_t c = (units + BOOK_CHUNKS_MAX - 1) / BOOK_CHUNKS_MAX;
    c = (c + GROUP - 1) / GROUP * GROUP;
    c = c < book_chunk_min(npb) ? book_chunk_min(npb) : c;
    return c < (1ull << 31) ? c : (1ull << 31);
}
// The chunks of one valid entry, in unit order (emit(unit, units, mask) for each; mask 0 = whole units); returns their count
template <class Emit>
static uint32_t book_entry_chunks(uint64_t first, uint64_t n, uint32_t npb, Emit emit)
{
    const uint64_t end = first + n, head = first / npb, tail_unit = end / npb, u0 = (first + npb - 1) / npb, u1 = end / npb;
    const bool has_head = first % npb != 0, has_tail = end % npb != 0 && !(has_head && tail_unit == head);
    const auto bits = [&](uint64_t unit) {   // the unit's paths inside [first, end)
        uint32_t m = 0;
        for (uint32_t j = 0; j < npb; ++j)
            m |= (unit * npb + j >= first && unit * npb + j < end) ? 1u << j : 0u;
        return m;
    };
    uint32_t count = 0;
    if (has_head)
        emit(head, 1, bits(head)), ++count;
    const uint64_t cu = book_chunk_units(u1 > u0 ? u1 - u0 : 0, npb);
    for (uint64_t u = u0; u < u1; ++count) {
        const uint64_t seam = ((u >> 32) + 1) << 32;
        uint64_t next = u + cu;
        next = next < u1 ? next : u1;
        next = next < seam ? next : seam;
        emit(u, next - u, 0u);
        u = next;
    }
    if (has_tail)
        emit(tail_unit, 1, bits(tail_unit)), ++count;
    return count;
}
static BookRefusal book_plan(const BookRange *r, int count, uint32_t npb, BookPlan &p)
{
    p.chunks.clear(), p.spans.clear(), p.counter_words = 0, p.bad_entry = -1;
    // first pass: every entry valid, and the book's chunk count within BOOK_MAX_CHUNKS -- before anything is stored
    uint64_t total = 0;
    for (int e = 0; e < count; ++e) {
        const uint64_t first = r[e].first_path, n = r[e].n_paths, end = first + n;
        BookRefusal why = n == 0 ? BOOK_EMPTY : (end < first ? BOOK_OVERFLOW : (n > (1ull << 52) ? BOOK_TOO_MANY_PATHS : BOOK_OK));
        const uint64_t u0 = (first + npb - 1) / npb, u1 = end / npb;
        if (why == BOOK_OK && u1 > u0) {   // plan_segments' rule (mc_api.hip): segments of <= 2^31 units, none across 2^32
            int segs = 0;
            for (uint64_t u = u0; u < u1 && segs <= MAX_SEGMENTS; ++segs) {
                const uint64_t room = (1ull << 32) - (u & 0xFFFFFFFFull), left = u1 - u;
                uint64_t m = left < room ? left : room;
                u += m < (1ull << 31) ? m : (1ull << 31);
            }
            if (segs > MAX_SEGMENTS)
                why = BOOK_TOO_MANY_SEGMENTS;
        }
        if (why == BOOK_OK) {
            total += book_entry_chunks(first, n, npb, [](uint64_t, uint64_t, uint32_t) {});
            if (total > BOOK_MAX_CHUNKS)
                why = BOOK_TOO_MANY_CHUNKS;
        }
        if (why != BOOK_OK) {
            p.bad_entry = e;
            return why;
        }
    }
    p.chunks.reserve((size_t)total);
    p.spans.reserve((size_t)count);
    for (int e = 0; e < count; ++e) {
        BookSpan s = {(uint32_t)p.chunks.size(), 0, 0, 0};
        s.chunks = book_entry_chunks(r[e].first_path, r[e].n_paths, npb, [&](uint64_t unit, uint64_t units, uint32_t mask) {
            p.chunks.push_back({(uint32_t)unit, (uint32_t)(unit >> 32), (uint32_t)units, (uint32_t)e, (uint32_t)(p.chunks.size() - s.chunk0), mask, 0u, 0u});   // seeds: the caller
        });
        s.shards = (s.chunks + BOOK_SHARD_CHUNKS - 1) / BOOK_SHARD_CHUNKS;
        if (s.shards == 1) {
            s.counter0 = p.counter_words++;
        } else {   // shards + 1 words, one 128-byte line each (mc_reduce.hpp TICKET_STRIDE)
            s.counter0 = (p.counter_words + TICKET_STRIDE - 1) / TICKET_STRIDE * TICKET_STRIDE;
            p.counter_words = s.counter0 + (s.shards + 1) * TICKET_STRIDE;
        }
        p.spans.push_back(s);
    }
    return BOOK_OK;
}

// How many pieces the fused kernels cut every reference thread's stream into (mc_grid.hpp "sub-streams"): enough to put
// ~8 waves on every SIMD (the reference's 512 x 128 launch alone is ONE), as long as a piece keeps >= 16 paths; a power
// of two up to 32.  MC_GRID_SUB forces a count (1 = the reference's own layout).
static void grid_pieces(int num_blocks, int num_threads, uint64_t paths_per_block, uint32_t *sub, uint32_t *seg)
{
    static const int forced = env_int("MC_GRID_SUB", 0, 0, 32);
    const uint64_t n_max = (paths_per_block + (uint64_t)num_threads - 1) / (uint64_t)num_threads;   // thread 0's paths
    const uint64_t lanes = (uint64_t)num_blocks * (uint64_t)((num_threads + 63) / 64 * 64), want = 8ull * 1024 * 64;
    uint32_t s = 1;
    if (forced > 0) {
        while (s * 2 <= (uint32_t)forced) s *= 2;
    } else {
        while (s < 32 && lanes * s * 2 <= want && n_max >= 16ull * s * 2)
            s *= 2;
    }
    const uint64_t per = (n_max + s - 1) / s;
    *sub = s;
    *seg = (uint32_t)((per + GRID_SEG_ALIGN - 1) / GRID_SEG_ALIGN * GRID_SEG_ALIGN);
}

}  // namespace mc
