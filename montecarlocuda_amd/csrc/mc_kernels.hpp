// mc_kernels.hpp -- the simulation kernels (gfx950, wave64).
//
// Shape common to all three products (replaces the kernel skeleton of
// dp/MonteCarloKernel.cu:133-177,179-220,222-283):
//   * a persistent-style grid (blocks x 256 lanes) strides over "units" of work; a unit is one
//     block of vanilla paths (4 in f32 = one Philox block, 8 in f64 = three) or one whole basket / CVA path;
//   * everything a lane needs is in registers: counter-based normals (mc_rng.hpp), per-lane fp64
//     (sum, sum2) accumulators; wave-uniform constants never cost a VALU slot -- kernel arguments in
//     SGPRs while they fit, otherwise LDS-staged (broadcast ds_read) or fetched tile by tile with
//     scalar loads from constant memory (the basket kernels), per-date rows through scalar loads (CVA);
//   * one DPP+LDS reduction and one 16-byte store per workgroup at the end; the last workgroup of the call to
//     arrive adds the pairs and writes the call's {sum, sum2, n} (mc_reduce.hpp: finish_group).
// HBM traffic per launch: kernel arguments (and a table of <= 20 KB) in, 16 B per workgroup out --
// the kernels are bound by VALU/transcendental issue, not by memory (DESIGN.md "Roofline").
//
// Work (one segment of units) and the generator policies (`Gen`: where the normals come from): mc_rng.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mc_reduce.hpp"
#include "mc_rng.hpp"

namespace mc {

constexpr int GROUP = 256;  // lanes per workgroup = 4 waves = one wave per SIMD

// precision-generic fused multiply-add (__builtin_fma alone is the double form)
__device__ __forceinline__ float fma_r(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_r(double a, double b, double c) { return __builtin_fma(a, b, c); }

__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 bcast(float x) { return (f2){x, x}; }
__device__ __forceinline__ f2 pk_exp2(f2 x) { return (f2){__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)}; }

// =========================================================================================
// Vanilla call.  Reference device formula, dp/MonteCarloKernel.cu:67-71:
//     payoff = max(S exp((r - v^2/2) T + v sqrt(T) z) - K, 0)
// =========================================================================================

// f32 constants, all prepared in fp64 on the host (mc_api.hip VanillaTraits<float>::prepare):
//   payoff = S 2^k * clamp(2^(a2k + b2 z) - kappa_k, 0, 1)
//   a2k = (r - v^2/2) T log2(e) - k,  b2 = v sqrt(T) log2(e),  kappa_k = (K/S) 2^-k,
//   radius2 = -2 ln2 * b2^2  (folds b2 into Box-Muller's radius: one fma per path after its normal)
//   k = integer with 2^(a2k + b2 |z|) <= 1 for every z the generator can produce (|z| < 6.77):
//       the payoff's max(.,0) then rides on the subtract as the free [0,1] output clamp
//       (v_sub_f32 ... clamp) instead of a separate v_max_f32; 2^k is exact, so the scaling
//       costs no precision.  Sums are scaled back by S 2^k and (S 2^k)^2 in the finishing kernel.
struct VanillaF32 {
    float a2k, radius2, kappa_k;
    float b2;   // read by the external-normals form only (the hot form has it folded into radius2)
};
struct VanillaF64 {
    double drift, vol, strike, spot;
};

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

// clamp(a + b, 0, 1) for BOTH halves of a packed pair in ONE instruction: v_pk_add_f32 with the output clamp.  hipcc
// never selects it (a packed min/max pair becomes two v_pk ops plus two scalar v_max ... clamp), hence the asm.  The
// fp32 vanilla payoffs max(2^x - kappa, 0) of two paths cost one issue slot this way instead of two v_sub_f32 ... clamp
// (63 -> 61 VALU instructions per Philox block; -2.7 % time, profiles/r02_ab_packed_clamp.log).  Not used in the basket
// kernels: there the "v" operands push wave-uniform constants out of the scalar registers and cost more v_readlane than
// the packing saves (145 -> 152 at n = 4).
__device__ __forceinline__ f2 pk_add_clamp01(f2 a, f2 b)
{
    // s_nop 0: gfx950 needs one wait state between a transcendental (the v_exp_f32 that produced `a`) and a VALU
    // instruction reading its result; hipcc inserts it for its own instructions but does not look inside an asm
    // (without it the antithetic kernel read a stale exponential: caught by test_vanilla_many_trips_vs_oracle)
    f2 r;
    asm("s_nop 0\n\tv_pk_add_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Box-Muller for the packed-fp32 kernels: the two word pairs (xa, ya) and (xb, yb) -- one Philox block's two pairs in
// the vanilla kernel, the same pair of TWO paths' blocks in the basket kernels -- as the halves of packed registers, so
// the uniform scaling, the radius scaling and z = r trig issue as v_pk_*_f32 (2 results per 4-cycle issue slot).
// Returns the radius {a, b} scaled by sqrt(scale2 / (-2 ln 2)) and the trig values; callers form z = r c, r s (or fold
// them into an fma).  v_log_f32 is log2 and v_sin/v_cos_f32 take revolutions: 2 pi never appears.
__device__ __forceinline__ void box_muller_pk(uint32_t xa, uint32_t ya, uint32_t xb, uint32_t yb, float scale2, f2 &rad, f2 &c, f2 &s)
{
    const f2 ua = pk_fma((f2){(float)xa, (float)xb}, bcast(0x1p-32f), bcast(0x1p-33f));  // radius uniforms
    const f2 ub = {angle_f32(ya), angle_f32(yb)};                                        // angle uniforms (revolutions, in [1, 2))
    const f2 t = (f2){__builtin_amdgcn_logf(ua.x), __builtin_amdgcn_logf(ua.y)} * bcast(scale2);
    rad = (f2){__builtin_amdgcn_sqrtf(t.x), __builtin_amdgcn_sqrtf(t.y)};
    c = (f2){__builtin_amdgcn_cosf(ub.x), __builtin_amdgcn_cosf(ub.y)};
    s = (f2){__builtin_amdgcn_sinf(ub.x), __builtin_amdgcn_sinf(ub.y)};
}

// The 4 scaled payoffs of one unit (one Philox block).  Box-Muller pair A = words (x, y), pair B = words
// (z, w); values are kept as {A, B} register pairs:
//   pc = cos-branch payoffs {A, B} = paths 4q+0, 4q+2;  ps = sin-branch {A, B} = paths 4q+1, 4q+3
// b2 is folded into the radius (o.radius2), so a path's exponent is ONE fma after its trig value.
//
// ANTI = antithetic variates (not in the reference): every normal z also prices the
// mirrored path -z; the sample is the mean of the two payoffs (here their sum: the 1/2 rides on the
// finishing step's scale).  Costs one more fma + exponential + clamp-subtract per path.
//
// GenExternal (from-normals hooks, launch-geometry mode): the four normals come from memory and the exponent is fma(z, b2, a2k); everything after the
// exponent -- exponential, clamp-subtract, sums, flushes, final reduction -- is the code of the hot path.
//
// `r` = the unit's four words when the caller has them already (vanilla_f32_blocked_kernel), else drawn from `gen`.
template <bool ANTI, class Gen>
__device__ __forceinline__ void vanilla_unit_pk(Gen &gen, const VanillaF32 &o, const Work &w, uint32_t c0, f2 &pc, f2 &ps, const u32x4 *have = nullptr)
{
    const f2 a = bcast(o.a2k);
    f2 yc, ys, mc_, ms_;   // exponents (log2 units) of the cos / sin branch paths and of their mirrors
    if constexpr (Gen::external) {
        float z[4];
        gen.normals(w, c0, 0u, 1u /*MC_DOMAIN_VANILLA*/, z);
        const f2 zc = {z[0], z[2]}, zs = {z[1], z[3]}, b = bcast(o.b2);
        yc = pk_fma(zc, b, a), ys = pk_fma(zs, b, a);
        mc_ = pk_fma(-zc, b, a), ms_ = pk_fma(-zs, b, a);
    } else {
        const u32x4 r = have ? *have : gen.words(w, c0, 0u, 1u /*MC_DOMAIN_VANILLA*/);
        f2 rad, c, s;
        box_muller_pk(r.x, r.y, r.z, r.w, o.radius2, rad, c, s);
        yc = pk_fma(c, rad, a), ys = pk_fma(s, rad, a);
        mc_ = pk_fma(-c, rad, a), ms_ = pk_fma(-s, rad, a);
    }
    const f2 neg_kappa = bcast(-o.kappa_k);
    pc = pk_add_clamp01(pk_exp2(yc), neg_kappa);
    ps = pk_add_clamp01(pk_exp2(ys), neg_kappa);
    if (ANTI) {
        pc += pk_add_clamp01(pk_exp2(mc_), neg_kappa);
        ps += pk_add_clamp01(pk_exp2(ms_), neg_kappa);
    }
}

// path order inside the unit: 4q+0 = cos A, 4q+1 = sin A, 4q+2 = cos B, 4q+3 = sin B
template <bool ANTI, class Gen>
__device__ __forceinline__ void vanilla_unit(Gen &gen, const VanillaF32 &o, const Work &w, uint32_t c0, float (&p)[4])
{
    f2 pc, ps;
    vanilla_unit_pk<ANTI>(gen, o, w, c0, pc, ps);
    p[0] = pc.x;
    p[1] = ps.x;
    p[2] = pc.y;
    p[3] = ps.y;
}
template <bool ANTI, class Gen, int NPB>
__device__ __forceinline__ void vanilla_unit(Gen &gen, const VanillaF64 &o, const Work &w, uint32_t c0, double (&p)[NPB])
{
    double z[NPB];
    gen.normals(w, c0, 0u, 1u /*MC_DOMAIN_VANILLA*/, z);
#pragma unroll
    for (int j = 0; j < NPB; ++j) {
        p[j] = fmax(o.spot * exp_f64(o.drift + o.vol * z[j]) - o.strike, 0.0);
        if (ANTI)
            p[j] = 0.5 * (p[j] + fmax(o.spot * exp_f64(o.drift - o.vol * z[j]) - o.strike, 0.0));
    }
}

// Hot kernels: every unit is complete.
//
// f32: per-lane sums live in two packed-f32 pairs for FLUSH iterations (16 values per fp32
// accumulator) and are then flushed to the lane's fp64 accumulators -- never a long fp32 running
// sum.  The trip count is wave-uniform (scalar loop control); the one partial
// trip at the end is peeled.
constexpr uint32_t VANILLA_F32_FLUSH = 8;

template <bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void vanilla_f32_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const VanillaF32 o, const Work w)
{
    const uint32_t stride = gridDim.x * GROUP;
    const uint32_t gtid = blockIdx.x * GROUP + threadIdx.x;
    const uint32_t full_trips = w.n_units / stride;
    double acc_s = 0.0, acc_q = 0.0;
    f2 s2 = {0.0f, 0.0f}, q2 = {0.0f, 0.0f};
    uint32_t c0 = w.unit_lo + gtid;
    Gen gen(w);   // Philox: stateless; XORWOW: the lane's sequence (units ascending, as the masked kernel draws them)
    for (uint32_t trip = 0; trip < full_trips; ++trip, c0 += stride) {
        f2 pc, ps;
        vanilla_unit_pk<ANTI>(gen, o, w, c0, pc, ps);
        s2 += pc;
        s2 += ps;
        q2 = pk_fma(pc, pc, q2);
        q2 = pk_fma(ps, ps, q2);
        if ((trip & (VANILLA_F32_FLUSH - 1)) == VANILLA_F32_FLUSH - 1) {
            acc_s += (double)(s2.x + s2.y);
            acc_q += (double)(q2.x + q2.y);
            s2 = (f2){0.0f, 0.0f};
            q2 = (f2){0.0f, 0.0f};
        }
    }
    if (full_trips * stride + gtid < w.n_units) {  // the partial last trip
        f2 pc, ps;
        vanilla_unit_pk<ANTI>(gen, o, w, c0, pc, ps);
        s2 += pc + ps;
        q2 += pc * pc + ps * ps;
    }
    acc_s += (double)(s2.x + s2.y);
    acc_q += (double)(q2.x + q2.y);
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// f32, Philox, LARGE calls: a lane takes whole 8-aligned BLOCKS of 8 consecutive units, lane g blocks g, g + stride, ...
// (a SWEEP of the grid = 8 stride units).  The eight units share the front of Philox (mc_rng.hpp: PhiloxBlock8), a block is
// exactly one flush group -- its first unit initialises the fp32 partials, its end flushes them: no zeroing, no per-trip
// flush test -- and the counter moves once per block: 481 VALU instructions per 8 units against the loop above's 500.  Same
// payoffs bit for bit, added up in another grouping.  Which units run blocked is the host's decision (mc_launch_shape.hpp:
// vanilla_blocking; it launches this kernel only where that pays): `sweeps` full sweeps, then lanes below `extra` take one
// more block (the last, partial sweep); the units outside the blocks -- `head` of them below the first multiple of 8, the
// others beyond the last block -- are unit-strided by the loop above, from the last lane down (those lanes took no block
// in a partial sweep), `rest_trips` full trips and a partial one.
struct VanillaBlocking {
    uint32_t head;         // leading units below the first multiple of 8
    uint32_t sweeps;       // full sweeps of blocks
    uint32_t extra;        // blocks of the last, partial sweep; 0 = none
    uint32_t blocked;      // units in blocks = 8 (sweeps stride + extra); 0 = the call runs vanilla_f32_kernel
    uint32_t rest_trips;   // full unit-strided trips over the units beyond the last block: (n_units - head - blocked) / stride
};

// one unit into the fp32 partials; FIRST: the unit that begins a flush group initialises them (the same bits as adding to 0)
template <bool FIRST> __device__ __forceinline__ void vanilla_f32_add(f2 pc, f2 ps, f2 &s2, f2 &q2)
{
    if constexpr (FIRST) {
        s2 = pc + ps;
        q2 = pk_fma(ps, ps, pc * pc);
    } else {
        s2 += pc;
        s2 += ps;
        q2 = pk_fma(pc, pc, q2);
        q2 = pk_fma(ps, ps, q2);
    }
}

// the 8 units of the block at `base` (8-aligned), flushed into the fp64 accumulators
template <bool ANTI>
__device__ __forceinline__ void vanilla_f32_block(GenPhilox &gen, const PhiloxBlock8 &px, const VanillaF32 &o, const Work &w, uint32_t base,
                                                  double &acc_s, double &acc_q)
{
    const uint64_t shared = px.shared(base);
    f2 s2, q2;
    const auto unit = [&](auto l) {
        constexpr int L = decltype(l)::value;
        const u32x4 r = px.template words<L>(shared);
        f2 pc, ps;
        vanilla_unit_pk<ANTI>(gen, o, w, base, pc, ps, &r);
        vanilla_f32_add<L == 0>(pc, ps, s2, q2);
    };
    unit(std::integral_constant<int, 0>()), unit(std::integral_constant<int, 1>()), unit(std::integral_constant<int, 2>());
    unit(std::integral_constant<int, 3>());
    // left alone the scheduler issues all seven addend multiplies up front and runs out of registers (a spill in the loop):
    // the second half of the block is scheduled on its own
    __builtin_amdgcn_sched_barrier(0);
    unit(std::integral_constant<int, 4>()), unit(std::integral_constant<int, 5>());
    unit(std::integral_constant<int, 6>()), unit(std::integral_constant<int, 7>());
    static_assert(VANILLA_F32_FLUSH == 8, "a block is one flush group");
    acc_s += (double)(s2.x + s2.y);
    acc_q += (double)(q2.x + q2.y);
}

template <bool ANTI>
__global__ __launch_bounds__(GROUP) void vanilla_f32_blocked_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const VanillaF32 o, const Work w,
                                                                    const VanillaBlocking b)
{
    const uint32_t stride = gridDim.x * GROUP;
    uint32_t gtid = blockIdx.x * GROUP + threadIdx.x;
    double acc_s = 0.0, acc_q = 0.0;
    GenPhilox gen(w);
    const PhiloxBlock8 px(w.unit_hi, 0u, 1u /*MC_DOMAIN_VANILLA*/, w.seed_lo, w.seed_hi);
    uint32_t base = w.unit_lo + b.head + (gtid << 3);
    for (uint32_t sweep = 0; sweep < b.sweeps; ++sweep, base += stride << 3)
        vanilla_f32_block<ANTI>(gen, px, o, w, base, acc_s, acc_q);
    // the lane's index again, from its block counter: one register less alive through the loop
    asm volatile("" : "+v"(base));
    gtid = (base - (w.unit_lo + b.head + ((b.sweeps * stride) << 3))) >> 3;
    if (gtid < b.extra)
        vanilla_f32_block<ANTI>(gen, px, o, w, base, acc_s, acc_q);
    // the units beyond the last block, unit-strided from the last lane down (those lanes took no block in a partial sweep) ...
    const uint32_t tail0 = w.unit_lo + b.head + b.blocked, n_tail = w.n_units - b.head - b.blocked, lane = stride - 1u - gtid;
    f2 s2 = {0.0f, 0.0f}, q2 = {0.0f, 0.0f};   // at most 7 trips and a partial one: one flush group (the head units go to fp64 on their own)
    uint32_t c0 = tail0 + lane;
    for (uint32_t trip = 0; trip < b.rest_trips; ++trip, c0 += stride) {
        f2 pc, ps;
        vanilla_unit_pk<ANTI>(gen, o, w, c0, pc, ps);
        vanilla_f32_add<false>(pc, ps, s2, q2);
    }
    if (b.rest_trips * stride + lane < n_tail) {
        f2 pc, ps;
        vanilla_unit_pk<ANTI>(gen, o, w, c0, pc, ps);
        vanilla_f32_add<false>(pc, ps, s2, q2);
    }
    // ... and the `head` units below the first block, one each for the first lanes
    if (gtid < b.head) {
        f2 pc, ps;
        vanilla_unit_pk<ANTI>(gen, o, w, w.unit_lo + gtid, pc, ps);
        acc_s += (double)(pc.x + ps.x + pc.y + ps.y);
        acc_q += (double)(pc.x * pc.x + ps.x * ps.x + pc.y * pc.y + ps.y * ps.y);
    }
    acc_s += (double)(s2.x + s2.y);
    acc_q += (double)(q2.x + q2.y);
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// f64 (and the generic form): each unit's payoffs go straight into the fp64 accumulators.
template <class Opt, class Real, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void vanilla_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const Opt o, const Work w)
{
    stage_tables<Real>();
    constexpr int NPB = Gen::template npb<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    const uint32_t gtid = blockIdx.x * GROUP + threadIdx.x;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = gtid; i < w.n_units; i += stride) {
        Real p[NPB];
        vanilla_unit<ANTI>(gen, o, w, w.unit_lo + i, p);
        Real s = p[0], q = p[0] * p[0];
#pragma unroll
        for (int j = 1; j < NPB; ++j) {
            s += p[j];
            q = fma_r(p[j], p[j], q);
        }
        acc_s += (double)s;
        acc_q += (double)q;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// Masked kernel: honours the path window (partial first/last units) and optionally stores
// every per-path payoff (currency units) to `out[p - first_path]`.  Used for range edges and
// by the parity tests; never on the hot path.
template <class Opt, class Real, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void vanilla_masked_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const Opt o, const Work w,
                                                               Real *__restrict__ out, Real out_scale)
{
    stage_tables<Real>();
    constexpr int NPB = Gen::template npb<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    const uint32_t gtid = blockIdx.x * GROUP + threadIdx.x;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = gtid; i < w.n_units; i += stride) {
        Real p[NPB];
        vanilla_unit<ANTI>(gen, o, w, w.unit_lo + i, p);
        const uint64_t unit = ((uint64_t)w.unit_hi << 32) | (uint32_t)(w.unit_lo + i);
#pragma unroll
        for (int j = 0; j < NPB; ++j) {
            const uint64_t path = unit * NPB + j;
            if (path >= w.first_path && path < w.end_path) {
                acc_s += (double)p[j];
                acc_q += (double)p[j] * (double)p[j];
                if (out)
                    out[path - w.first_path] = p[j] * out_scale;
            }
        }
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// A book of vanilla calls in one launch (mc_vanilla_book_*).  The host (mc_launch_shape.hpp: book_plan) cuts every entry's
// unit range into CHUNKS: a single-unit masked chunk for a partial first or last unit, and between them chunks of whole units
// whose boundaries depend on the entry's own range only, none across a multiple of 2^32 units.  A persistent grid walks the
// chunk table (workgroup x takes chunks x, x + grid, ...); a chunk runs the code of the single call -- the same per-unit
// function, the hot loop for whole units (fp32: the 8-trip flush), the path-window mask for the edge units -- on 256 lanes,
// lane t taking units t, t + 256, ..., so its (sum, sum2) pair is the same bits whichever workgroup computes it.  Each chunk
// publishes its pair into a slot of its own (indexed by chunk) and draws a ticket on its entry's counter; the workgroup that
// completes an entry adds the entry's pairs in chunk order and writes the entry's triple (book_close).  The two-launch form
// (fused == 0) stores the pairs plainly and vanilla_book_finish_kernel closes the entries with the same book_close.
// =========================================================================================
struct BookChunk {        // 32 bytes: one scalar load
    uint32_t unit_lo, unit_hi, n_units;
    uint32_t entry;       // index in the book
    uint32_t index;       // chunk number within the entry (its ticket shard: index % shards)
    uint32_t masked;      // 0: whole units; an edge unit: bit j set = path j of the unit is in the entry's range
    uint32_t seed_lo, seed_hi;   // the entry's seed (the loop reads nothing of the entry but its seed and option constants)
};
struct BookHead {         // what the closing needs, and the entry's generator inputs
    double scale1, scale2, n_paths;   // triple = {scale1 sum, scale2 sum2, n_paths}
    uint64_t first_path, end_path;    // the entry's range (the masked chunks carry it as a bit mask)
    uint32_t seed_lo, seed_hi;        // (the chunks carry copies)
    uint32_t chunk0, chunks;          // the entry's chunks (and pair slots) are chunk0 .. chunk0 + chunks - 1
    uint32_t shards, counter0;        // ticket words: counter0 (one shard); or shards + 1 words TICKET_STRIDE apart, the top word last
};
struct BookOut {          // the FIRST argument of the book kernels, read late (book_out_late) as the Tail is (mc_reduce.hpp: late_tail)
    const BookHead *heads;   // the entries' heads: read by the closing only
    double2 *pairs;       // one pair slot per chunk
    uint32_t *counters;   // all zero between calls (zeroed at allocation, reset by every closer)
    double *triples;      // 3 doubles per entry
    uint32_t fused;       // 0: plain pair stores, vanilla_book_finish_kernel follows
};
typedef const __attribute__((address_space(4))) BookOut *book_out_t;
__device__ __forceinline__ book_out_t book_out_late(double after)
{
    unsigned long long p = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p) : "v"(after));
    return (book_out_t)p;
}

// the Work of a chunk: the entry's seed, the chunk's units
__device__ __forceinline__ Work book_work(const BookChunk &ch)
{
    Work w;
    w.seed_lo = ch.seed_lo, w.seed_hi = ch.seed_hi;
    w.unit_lo = ch.unit_lo, w.unit_hi = ch.unit_hi, w.n_units = ch.n_units;
    w.first_path = w.end_path = 0;   // unused: a masked chunk carries its window as a bit mask
    w.xorwow = nullptr, w.ext = nullptr, w.ext_per_unit = 0;
    return w;
}

// Every lane: the entry's pairs in chunk order (lane t adds pairs t, t + 256, ...), the DPP/LDS reduction, the triple.
__device__ __forceinline__ void book_close(const double2 *pairs, const BookHead &h, double *triple)
{
    double s = 0.0, q = 0.0;
    for (uint32_t i = threadIdx.x; i < h.chunks; i += GROUP) {
        const double2 p = pairs[h.chunk0 + i];
        s += p.x;
        q += p.y;
    }
    group_sum2(s, q);
    if (threadIdx.x == 0) {
        triple[0] = h.scale1 * s;
        triple[1] = h.scale2 * q;
        triple[2] = h.n_paths;
    }
}

// The tables are read through the constant address space (scalar loads: chunk, head and option constants are wave-uniform).  The kernel
// never writes them; the host uploads them before the launch.
typedef const __attribute__((address_space(4))) BookChunk *book_chunks_t;
typedef const __attribute__((address_space(4))) BookHead *book_heads_t;
// C++ copies no struct out of another address space: field by field (each a scalar load)
__device__ __forceinline__ BookChunk book_load(book_chunks_t p)
{
    return {p->unit_lo, p->unit_hi, p->n_units, p->entry, p->index, p->masked, p->seed_lo, p->seed_hi};
}
__device__ __forceinline__ BookHead book_load(book_heads_t p)
{
    return {p->scale1, p->scale2, p->n_paths, p->first_path, p->end_path, p->seed_lo, p->seed_hi, p->chunk0, p->chunks, p->shards, p->counter0};
}
// After group_sum2 of chunk `ci`: publish its pair and, in the fused form, draw the entry's ticket; the workgroup that completes the
// entry closes it.  The protocol of arrive_and_finish (mc_reduce.hpp): write-through pair stores -> s_waitcnt vmcnt(0) -> relaxed
// agent-scope fetch_add on shard index % shards; the arrival that completes its shard adds 1 to the top word (entries of more than
// one shard), the one that completes that is the closer: agent-scope acquire -> plain loads.  A shard takes at most BOOK_SHARD_CHUNKS
// arrivals and the top word at most ~BOOK_CHUNKS_MAX / BOOK_SHARD_CHUNKS (mc_launch_shape.hpp).
__device__ __forceinline__ void book_arrive(uint32_t ci, book_chunks_t chunks, double s, double q)
{
    const book_out_t po = book_out_late(s);
    const BookOut out = {po->heads, po->pairs, po->counters, po->triples, po->fused};
    const BookChunk ch = book_load(chunks + ci);
    const BookHead h = book_load((book_heads_t)out.heads + ch.entry);
    __shared__ uint32_t lds_close;
    if (threadIdx.x == 0) {
        if (!out.fused) {
            out.pairs[ci] = make_double2(s, q);
        } else {   // write-through: the bytes leave this XCD's L2 (which no other XCD can see into)
            gu64_t *g = (gu64_t *)(out.pairs + ci);
            __hip_atomic_store(g, (unsigned long long)__double_as_longlong(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(g + 1, (unsigned long long)__double_as_longlong(q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the pair stores have left before the ticket is drawn
            const uint32_t shard = ch.index % h.shards, in_shard = (h.chunks - shard + h.shards - 1) / h.shards;
            const uint32_t stride = h.shards > 1 ? TICKET_STRIDE : 1;   // the words of a sharded entry: one 128-byte line each
            gu32_t *k = (gu32_t *)out.counters + h.counter0;
            uint32_t last = __hip_atomic_fetch_add(k + shard * stride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == in_shard;
            if (last && h.shards > 1)
                last = __hip_atomic_fetch_add(k + h.shards * stride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1 == h.shards;
            lds_close = last;
        }
    }
    if (!out.fused)
        return;
    __syncthreads();
    if (!lds_close)   // workgroup-uniform
        return;
    if (threadIdx.x == 0)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // drop this CU's stale lines of the pair buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    book_close(out.pairs, h, out.triples + 3 * (size_t)ch.entry);
    if (threadIdx.x < h.shards + (h.shards > 1 ? 1u : 0u))   // ready for the next call
        __hip_atomic_store((gu32_t *)out.counters + h.counter0 + threadIdx.x * (h.shards > 1 ? TICKET_STRIDE : 1), 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// A masked chunk (one edge unit) runs the same loop; the payoffs of the paths outside the entry's range are zeroed before they are added.
template <class Real> __device__ __forceinline__ Real book_window(Real p, uint32_t mask, int j) { return ((mask >> j) & 1u) ? p : (Real)0; }

// fp32: vanilla_f32_kernel's loop (packed pairs, the 8-trip flush), with lanes striding one workgroup
template <bool ANTI>
__global__ __launch_bounds__(GROUP) void vanilla_book_f32_kernel(const BookOut /* first argument, read late */, const BookChunk *chunk_table,
                                                                 const VanillaF32 *__restrict__ opt_table,
                                                                 uint32_t n_chunks)
{
    const book_chunks_t chunks = (book_chunks_t)chunk_table;
    for (uint32_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        const BookChunk ch = book_load(chunks + ci);
        const VanillaF32 &o = opt_table[ch.entry];   // a reference: a local copy becomes a per-lane LDS array (AMDGPUPromoteAlloca)
        const Work w = book_work(ch);
        GenPhilox gen(w);
        double acc_s = 0.0, acc_q = 0.0;
        const uint32_t full_trips = w.n_units / GROUP;
        f2 s2 = {0.0f, 0.0f}, q2 = {0.0f, 0.0f};
        uint32_t c0 = w.unit_lo + threadIdx.x;
        for (uint32_t trip = 0; trip < full_trips; ++trip, c0 += GROUP) {
            f2 pc, ps;
            vanilla_unit_pk<ANTI>(gen, o, w, c0, pc, ps);
            s2 += pc;
            s2 += ps;
            q2 = pk_fma(pc, pc, q2);
            q2 = pk_fma(ps, ps, q2);
            if ((trip & (VANILLA_F32_FLUSH - 1)) == VANILLA_F32_FLUSH - 1) {
                acc_s += (double)(s2.x + s2.y);
                acc_q += (double)(q2.x + q2.y);
                s2 = (f2){0.0f, 0.0f};
                q2 = (f2){0.0f, 0.0f};
            }
        }
        if (full_trips * GROUP + threadIdx.x < w.n_units) {   // the partial last trip (a masked chunk's one unit)
            f2 pc, ps;
            vanilla_unit_pk<ANTI>(gen, o, w, c0, pc, ps);
            if (ch.masked) {   // an edge unit, as vanilla_masked_kernel adds it: every live path in fp64
                const float p[4] = {pc.x, ps.x, pc.y, ps.y};   // path order inside the unit: 4q+0 .. 4q+3
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double x = book_window(p[j], ch.masked, j);
                    acc_s += x;
                    acc_q += x * x;
                }
            } else {
                s2 += pc + ps;
                q2 += pc * pc + ps * ps;
            }
        }
        acc_s += (double)(s2.x + s2.y);
        acc_q += (double)(q2.x + q2.y);
        group_sum2(acc_s, acc_q);
        book_arrive(ci, chunks, acc_s, acc_q);
    }
}

// fp64: vanilla_kernel's loop, with lanes striding one workgroup; the LDS tables are staged once per workgroup
template <class Real, bool ANTI>
__global__ __launch_bounds__(GROUP) void vanilla_book_kernel(const BookOut /* first argument, read late */, const BookChunk *chunk_table,
                                                             const VanillaF64 *__restrict__ opt_table,
                                                             uint32_t n_chunks)
{
    static_assert(sizeof(Real) == 8, "the fp32 book is vanilla_book_f32_kernel");
    stage_tables<Real>();
    constexpr int NPB = GenPhilox::npb<Real>();
    const book_chunks_t chunks = (book_chunks_t)chunk_table;
    for (uint32_t ci = blockIdx.x; ci < n_chunks; ci += gridDim.x) {
        const BookChunk ch = book_load(chunks + ci);
        const VanillaF64 &o = opt_table[ch.entry];   // a reference: a local copy becomes a per-lane LDS array (AMDGPUPromoteAlloca)
        const Work w = book_work(ch);
        GenPhilox gen(w);
        double acc_s = 0.0, acc_q = 0.0;
        for (uint32_t i = threadIdx.x; i < w.n_units; i += GROUP) {
            Real p[NPB];
            vanilla_unit<ANTI>(gen, o, w, w.unit_lo + i, p);
            if (ch.masked) {   // an edge unit (the chunk's only one)
#pragma unroll
                for (int j = 0; j < NPB; ++j)
                    p[j] = book_window(p[j], ch.masked, j);
            }
            Real s = p[0], q = p[0] * p[0];
#pragma unroll
            for (int j = 1; j < NPB; ++j) {
                s += p[j];
                q = fma_r(p[j], p[j], q);
            }
            acc_s += (double)s;
            acc_q += (double)q;
        }
        group_sum2(acc_s, acc_q);
        book_arrive(ci, chunks, acc_s, acc_q);
    }
}

// Two-launch form: workgroup x closes entries x, x + grid, ... from the pairs the simulation kernel stored
__global__ __launch_bounds__(GROUP) void vanilla_book_finish_kernel(const BookHead *__restrict__ heads, uint32_t count, const double2 *pairs,
                                                                    double *triples)
{
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const BookHead h = heads[e];
        book_close(pairs, h, triples + 3 * (size_t)e);
    }
}

// =========================================================================================
// Vanilla call with its Greeks (the reference prices only).  Per path, on the same normal as the pricing kernels:
//     S_T = S exp(drift + vol z),   I = [S_T > K],   payoff = I (S_T - K)
// in one of three forms (GreeksForm):
// PATHWISE:          d payoff / dS = I S_T / S,   d payoff / d sigma = I S_T (sqrt(T) z - sigma T)
// LIKELIHOOD_RATIO:  differentiate the lognormal density instead of the payoff (no indicator, so they also serve payoffs with
//                    jumps); with lr_delta = 1 / (S sigma sqrt T), inv_sigma = 1 / sigma:
//     delta = payoff z / (S sigma sqrt T),   vega = payoff ((z^2 - 1) / sigma - z sqrt T)
// SECOND_ORDER:      the pathwise delta and vega, and gamma and vanna by the mixed estimator (Glasserman 7.3: the likelihood-ratio
//                    derivative of the pathwise first derivative -- no indicator is differentiated twice, and the variance stays far
//                    below a pure likelihood-ratio second derivative); with dl = I S_T / S the pathwise delta, inv_spot = 1 / S:
//     gamma = dl (z lr_delta - inv_spot)                    = I S_T / S^2 (z / (sigma sqrt T) - 1)
//     vanna = dl (z (z inv_sigma - sqrt T) - inv_sigma)     = I S_T / S ((z^2 - 1) / sigma - z sqrt T)
// One (sum, sum2) pair per workgroup and plane of the call's pair buffer: price, delta, vega (, gamma, vanna).  Always honours
// the path window (no separate hot variant: a secondary kernel).
// =========================================================================================
struct GreeksF32 { float drift2, vol2, spot, strike, sqrt_t, sigma_t, lr_delta, inv_sigma; };   // exponent in log2 units
struct GreeksF64 { double drift, vol, spot, strike, sqrt_t, sigma_t, lr_delta, inv_sigma; };
enum GreeksForm { PATHWISE, LIKELIHOOD_RATIO, SECOND_ORDER };
constexpr int greeks_planes(GreeksForm f) { return f == SECOND_ORDER ? 5 : 3; }

__device__ __forceinline__ float greeks_spot(const GreeksF32 &o, float z) { return o.spot * __builtin_amdgcn_exp2f(__builtin_fmaf(o.vol2, z, o.drift2)); }
__device__ __forceinline__ double greeks_spot(const GreeksF64 &o, double z) { return o.spot * exp_f64(__builtin_fma(o.vol, z, o.drift)); }

// inv_spot = 1 / S: an argument of the SECOND_ORDER form only (the pack is empty in the first-order forms, whose kernel arguments
// stay (Tail, Opt, Work))
template <class Opt, class Real, GreeksForm F, class... InvSpot>
__global__ __launch_bounds__(GROUP) void vanilla_greeks_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const Opt o, const Work w,
                                                               const InvSpot... inv_spot)
{
    stage_tables<Real>();
    constexpr int NPB = GenPhilox::npb<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc[2 * greeks_planes(F)] = {};
    GenPhilox gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        Real z[NPB];
        gen.normals(w, w.unit_lo + i, 0u, 1u /*MC_DOMAIN_VANILLA*/, z);
        const uint64_t unit = ((uint64_t)w.unit_hi << 32) | (uint32_t)(w.unit_lo + i);
#pragma unroll
        for (int j = 0; j < NPB; ++j) {
            const uint64_t path = unit * NPB + j;
            if (path >= w.first_path && path < w.end_path) {
                Real st = greeks_spot(o, z[j]);
                // In the first-order forms, fp32 S_T is rounded before every use (in fp64 the payoff is fma(S, e, -K)).  The second
                // order's extra uses of S_T and z let the compiler fuse differently in fp32, so there S_T is made opaque: price, delta
                // and vega stay the pathwise form's bits.
                if constexpr (F == SECOND_ORDER && sizeof(Real) == 4)
                    asm volatile("" : "+v"(st));
                const bool itm = st > o.strike;
                const Real payoff = itm ? st - o.strike : (Real)0;
                const double pay = (double)payoff;
                double dl, vg, gm, va;   // gm, va: SECOND_ORDER only
                if constexpr (F == LIKELIHOOD_RATIO) {
                    dl = (double)(payoff * z[j] * o.lr_delta);
                    vg = (double)(payoff * ((z[j] * z[j] - (Real)1) * o.inv_sigma - z[j] * o.sqrt_t));
                } else if constexpr (F == PATHWISE) {
                    dl = itm ? (double)(st / o.spot) : 0.0;
                    vg = itm ? (double)(st * (o.sqrt_t * z[j] - o.sigma_t)) : 0.0;
                } else {   // the pathwise delta and vega; vega's fma spelled out (the pathwise form's (sqrt_t z - sigma_t) contracts to it)
                    const Real d_r = st / o.spot;
                    dl = itm ? (double)d_r : 0.0;
                    vg = itm ? (double)(st * fma_r(o.sqrt_t, z[j], -o.sigma_t)) : 0.0;
                    gm = itm ? (double)(d_r * fma_r(z[j], o.lr_delta, -inv_spot...)) : 0.0;
                    va = itm ? (double)(d_r * fma_r(z[j], fma_r(z[j], o.inv_sigma, -o.sqrt_t), -o.inv_sigma)) : 0.0;
                }
                pair_add(acc, 0, pay);
                pair_add(acc, 1, dl);
                pair_add(acc, 2, vg);
                if constexpr (F == SECOND_ORDER) {
                    pair_add(acc, 3, gm);
                    pair_add(acc, 4, va);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < greeks_planes(F); ++q) {
        group_sum2(acc[2 * q], acc[2 * q + 1]);
        pair_publish(late_tail(acc[2 * q]), acc, q, q);
    }
    arrive_and_finish(late_tail(acc[0]));
}

// =========================================================================================
// Basket call.  Reference device formulas, dp/MonteCarloKernel.cu:74-101:
//     bt = L g + d;  s_a = S_a exp((r - v_a^2/2) T + v_a sqrt(T) bt_a);
//     payoff = max(sum_a w_a s_a - K, 0)
// folded on the host (fp64) into  payoff = max(sum_a coef_a E(base_a + sum_{b<=a} m_ab g_b) - K, 0)
// with m = diag(v sqrt T) L (lower triangle only: the reference multiplies the structural
// zeros too, :79-84), base_a = (r - v_a^2/2) T + v_a sqrt(T) d_a, coef_a = w_a S_a;
// in f32 m and base are pre-multiplied by log2(e) and E = 2^x (v_exp_f32).
// =========================================================================================
template <class Real, int NA>
struct BasketArgs {
    Real m[NA * (NA + 1) / 2];  // packed rows: m[a(a+1)/2 + b], b <= a
    Real base[NA];
    Real coef[NA];
    Real strike;
    // geometric-basket control variate (off in the reference's plain estimator):
    // ln G = cg + sum_a wg_a x_a in the kernel's exponent units, x_a = asset a's exponent.  When
    // cv != 0 the per-path value is payoff(arithmetic) - payoff(geometric); the closed-form mean of
    // the latter (mc_basket_control_mean_*) is added back on the host.
    Real wg[NA];
    Real cg;
    int cv;
};

// Where a basket kernel reads its folded constants from.  Small baskets keep them in SGPRs straight from
// the kernel arguments; larger ones do not fit the scalar register file (hipcc then "spills" SGPRs into
// VGPR lanes and pays a v_readlane_b32 -- a full VALU issue slot -- per use: 272 of 870 instructions per
// trip at n=16 f32), so they are staged once per workgroup into LDS and read back as broadcast
// ds_reads, which do not occupy the VALU.
// Which sizes stage (in-process A/B on MI355X, tools/ab_basket.py, profiles/r01_ab_basket_lds.log; kernel time LDS vs
// SGPR constants):
//   f32  n=6 -1 %, n=8 -11 %, n=10 -15 % (no fence);  n=12 -15 %, n=16 -20 % (fence every 4 rows; -6 % / -5 % without)
//   f64  n=4 -7 %, n=7 -10 %, n=8 -12 %, n=9 -11 %, n=10 +1 %, n=12 +2 %, n=16 +6 % (no fence; a fence costs f64
//        3-9 %).  From n=10 hipcc keeps the staged constants in > 256 registers: one wave per SIMD, every LDS
//        latency exposed; asking for more waves (amdgpu_waves_per_eu) turns that into scratch spills, so those
//        sizes stay on the SGPR path (and run the tiled kernels by default: mc_api.hip).
template <class Real, int NA> constexpr bool basket_consts_in_lds()
{
    return sizeof(Real) == 4 ? NA > 5 : (NA > 3 && NA <= 9);
}
// Whether the LDS reads are additionally pinned every few rows (ConstsLds::fence): the fence period in rows (0 = never).
template <class Real, int NA> constexpr int basket_fence_rows() { return sizeof(Real) == 4 && NA >= 11 ? 4 : 0; }

template <class Real, int NA>
struct ConstsArg {  // kernel arguments (SGPRs)
    const BasketArgs<Real, NA> &o;
    __device__ __forceinline__ Real m(int i) const { return o.m[i]; }
    __device__ __forceinline__ Real base(int a) const { return o.base[a]; }
    __device__ __forceinline__ Real coef(int a) const { return o.coef[a]; }
    __device__ __forceinline__ Real wg(int a) const { return o.wg[a]; }
    template <class T> __device__ __forceinline__ void fence(int, T) {}
};
template <class Real, int NA>
struct ConstsLds {  // staged copy: m | base | coef | wg
    static constexpr int NM = NA * (NA + 1) / 2, COUNT = NM + 3 * NA;
    const Real *p;
    int off = 0;  // always 0, but opaque to the compiler (see fence)
    __device__ __forceinline__ Real m(int i) const { return p[off + i]; }
    __device__ __forceinline__ Real base(int a) const { return p[off + NM + a]; }
    __device__ __forceinline__ Real coef(int a) const { return p[off + NM + NA + a]; }
    __device__ __forceinline__ Real wg(int a) const { return p[off + NM + 2 * NA + a]; }
    // The staged constants never change, so left alone hipcc hoists every ds_read out of the path loop
    // (or to the top of a trip) and pins ~140 values in VGPRs -- 168 VGPRs and scratch at n=16.  Tying
    // the read offset to the value computed just before (a row's exponent) keeps each row's reads next to
    // the row that uses them.
    template <class T> __device__ __forceinline__ void fence(int row, T dep)
    {
        constexpr int PERIOD = basket_fence_rows<Real, NA>();
        if (PERIOD > 0 && row % (PERIOD > 0 ? PERIOD : 1) == 0)  // row is a compile-time constant after unrolling
            asm volatile("" : "+v"(off) : "v"(dep));
    }
    // Thread 0 writes every constant with a compile-time index (SGPR -> v_mov -> ds_write): a per-thread
    // index into the kernel-argument struct would make hipcc copy the whole struct to scratch first.
    __device__ __forceinline__ static void stage(Real *lds, const BasketArgs<Real, NA> &o)
    {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < NM; ++i)
                lds[i] = o.m[i];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                lds[NM + a] = o.base[a];
                lds[NM + NA + a] = o.coef[a];
                lds[NM + 2 * NA + a] = o.wg[a];
            }
        }
        __syncthreads();
    }
};

__device__ __forceinline__ float exp_model(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ double exp_model(double x) { return exp_f64(x); }

// The end of a basket path, shared by every one-path-per-lane basket kernel: from the weighted sum of the terminal
// prices (and of the mirrored path's, ANTI) to the sample.  Reference: dp/MonteCarloKernel.cu:96-100.
//   cv (wave-uniform): geometric-basket control variate -- the sample is payoff(arithmetic) - payoff(geometric),
//   lg / lgm = ln G of the path and of its mirror in the kernel's exponent units.
template <bool ANTI, class Real>
__device__ __forceinline__ Real basket_sample(Real basket, Real mirror, Real lg, Real lgm, Real strike, int cv)
{
    const Real v = basket - strike;
    Real pay = v > 0 ? v : 0;
    if (cv) {
        const Real gv = exp_model(lg) - strike;
        pay -= gv > 0 ? gv : 0;
    }
    if (ANTI) {
        const Real vm = mirror - strike;
        Real pm = vm > 0 ? vm : 0;
        if (cv) {
            const Real gm = exp_model(lgm) - strike;
            pm -= gm > 0 ? gm : 0;
        }
        pay = (Real)0.5 * (pay + pm);
    }
    return pay;
}
// the same for two paths in packed halves (the fp32 tiled / generic kernels: plain max, no power-of-two rescale)
template <bool ANTI>
__device__ __forceinline__ f2 basket_sample_pk(f2 basket, f2 mirror, f2 lg, f2 lgm, float strike_, int cv)
{
    const f2 zero = {0.0f, 0.0f}, strike = bcast(strike_);
    f2 p = __builtin_elementwise_max(basket - strike, zero);
    if (cv)
        p -= __builtin_elementwise_max(pk_exp2(lg) - strike, zero);
    if (ANTI) {
        f2 pm = __builtin_elementwise_max(mirror - strike, zero);
        if (cv)
            pm -= __builtin_elementwise_max(pk_exp2(lgm) - strike, zero);
        p = bcast(0.5f) * (p + pm);
    }
    return p;
}

// One row of the folded model: the asset's exponent x is done; add its terminal price (and the mirrored path's, whose
// exponent is base - m g = 2 base - x) to the weighted sums, and its log to the control variate's.
// wg() yields the row's control-variate weight; it is only evaluated where it is used (for the LDS-staged constants it
// is a read), cv is wave-uniform.
template <bool ANTI, class Real, class Wg>
__device__ __forceinline__ void basket_row(Real x, Real base, Real coef, Wg wg, int cv, Real &basket, Real &mirror, Real &lg, Real &lgm)
{
    basket = fma_r(coef, exp_model(x), basket);
    if (cv)
        lg = fma_r(wg(), x, lg);
    if (ANTI) {
        const Real xm = fma_r((Real)-1, x, 2 * base);
        mirror = fma_r(coef, exp_model(xm), mirror);
        if (cv)
            lgm = fma_r(wg(), xm, lgm);
    }
}
template <bool ANTI, class Wg>
__device__ __forceinline__ void basket_row_pk(f2 x, float base, float coef, Wg wg, int cv, f2 &basket, f2 &mirror, f2 &lg, f2 &lgm)
{
    basket = pk_fma(bcast(coef), pk_exp2(x), basket);
    if (cv)
        lg = pk_fma(bcast(wg()), x, lg);
    if (ANTI) {
        const f2 xm = pk_fma(bcast(-1.0f), x, bcast(2.0f * base));
        mirror = pk_fma(bcast(coef), pk_exp2(xm), mirror);
        if (cv)
            lgm = pk_fma(bcast(wg()), xm, lgm);
    }
}

// All normals of one path: blocks 0 .. NBLK-1 of unit c0 in the basket domain
template <class Gen, class Real, int NG>
__device__ __forceinline__ void basket_normals(Gen &gen, const Work &w, uint32_t c0, Real (&g)[NG])
{
    constexpr int NPB = Gen::template npb<Real>();
    static_assert(NG % NPB == 0, "whole blocks");
#pragma unroll
    for (int b = 0; b < NG / NPB; ++b) {
        Real z[NPB];
        gen.normals(w, c0, (uint32_t)b, 2u /*MC_DOMAIN_BASKET*/, z);
#pragma unroll
        for (int j = 0; j < NPB; ++j)
            g[b * NPB + j] = z[j];
    }
}
// ... of TWO paths (units cA, cB) as packed halves {A, B}: the fp32 two-paths-per-lane kernels.  Blocks first_block ..
// first_block + NBLK - 1; dst(k) = where normal k of them goes (a register array or the lane's LDS column).
template <int NBLK, class Gen, class Dst>
__device__ __forceinline__ void basket_normals_pk(Gen &gen, const Work &w, uint32_t cA, uint32_t cB, Dst dst, uint32_t first_block = 0)
{
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
        if constexpr (Gen::external) {
            float za[4], zb[4];
            gen.normals(w, cA, first_block + (uint32_t)b, 2u /*MC_DOMAIN_BASKET*/, za);
            gen.normals(w, cB, first_block + (uint32_t)b, 2u, zb);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                dst(4 * b + j) = (f2){za[j], zb[j]};
        } else {
            const u32x4 ra = gen.words(w, cA, first_block + (uint32_t)b, 2u /*MC_DOMAIN_BASKET*/);
            const u32x4 rb = gen.words(w, cB, first_block + (uint32_t)b, 2u);
            // Box-Muller pair X = words (x, y), pair Z = words (z, w); halves = {path A, path B}
            f2 rx, cx, sx, rz, cz, sz;
            box_muller_pk(ra.x, ra.y, rb.x, rb.y, NEG_2LN2_F32, rx, cx, sx);
            box_muller_pk(ra.z, ra.w, rb.z, rb.w, NEG_2LN2_F32, rz, cz, sz);
            dst(4 * b + 0) = rx * cx;
            dst(4 * b + 1) = rx * sx;
            dst(4 * b + 2) = rz * cz;
            dst(4 * b + 3) = rz * sz;
        }
    }
}

template <class Real, int NA, bool ANTI, class Gen, class Consts>
__device__ __forceinline__ Real basket_path(Gen &gen, const BasketArgs<Real, NA> &o, Consts k, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<Real>();
    constexpr int NBLK = (NA + NPB - 1) / NPB;
    Real g[NBLK * NPB];
    basket_normals(gen, w, c0, g);
    Real basket = 0, mirror = 0, lg = o.cg, lgm = o.cg;
    k.fence(0, g[0]);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const Real base = k.base(a), coef = k.coef(a);
        Real x = base;
#pragma unroll
        for (int b = 0; b <= a; ++b)
            x = fma_r(k.m(a * (a + 1) / 2 + b), g[b], x);
        basket_row<ANTI>(x, base, coef, [&] { return k.wg(a); }, o.cv, basket, mirror, lg, lgm);
        k.fence(a + 1, x);
    }
    return basket_sample<ANTI>(basket, mirror, lg, lgm, o.strike, o.cv);
}

template <class Real, int NA, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void basket_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const BasketArgs<Real, NA> o, const Work w,
                                                       Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    const uint32_t gtid = blockIdx.x * GROUP + threadIdx.x;
    double acc_s = 0.0, acc_q = 0.0;
    constexpr bool IN_LDS = basket_consts_in_lds<Real, NA>();
    __shared__ Real lds_consts[IN_LDS ? ConstsLds<Real, NA>::COUNT : 1];
    if (IN_LDS)
        ConstsLds<Real, NA>::stage(lds_consts, o);
    Gen gen(w);
    for (uint32_t i = gtid; i < w.n_units; i += stride) {
        Real p;
        if constexpr (IN_LDS)
            p = basket_path<Real, NA, ANTI>(gen, o, ConstsLds<Real, NA>{lds_consts}, w, w.unit_lo + i);
        else
            p = basket_path<Real, NA, ANTI>(gen, o, ConstsArg<Real, NA>{o}, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// ---- f32 basket: TWO paths per lane, one in each half of a packed-f32 register pair ----------
// Everything that is not Philox or a transcendental (uniform scaling, radius scaling, z = r*trig,
// the whole triangular mat-vec, the weighted sum, the sums) issues as v_pk_*_f32: two paths per
// 4-cycle slot.  The payoff's max(.,0) is the free [0,1] clamp of the subtract after an exact
// power-of-two rescale (coef and strike carry 2^-k, k from the generator's |z| < 6.77 bound);
// the finishing kernel scales the sums back.  Lane pairing: units i and i + stride of one trip.
template <int NA, bool ANTI, class Gen, class Consts>
__device__ __forceinline__ f2 basket_pair_f32(Gen &gen, const BasketArgs<float, NA> &o, Consts k, const Work &w, uint32_t cA, uint32_t cB)
{
    constexpr int NBLK = (NA + 3) / 4;
    f2 g[NBLK * 4];
    basket_normals_pk<NBLK>(gen, w, cA, cB, [&](int i) -> f2 & { return g[i]; });
    f2 basket = {0.0f, 0.0f}, mirror = {0.0f, 0.0f}, lg = bcast(o.cg), lgm = bcast(o.cg);
    k.fence(0, g[0].x);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const float base = k.base(a), coef = k.coef(a);
        f2 x = bcast(base);
#pragma unroll
        for (int b = 0; b <= a; ++b)
            x = pk_fma(bcast(k.m(a * (a + 1) / 2 + b)), g[b], x);
        basket_row_pk<ANTI>(x, base, coef, [&] { return k.wg(a); }, o.cv, basket, mirror, lg, lgm);
        k.fence(a + 1, x.x);
    }
    // payoff = the free [0,1] clamp of the subtract after the power-of-two rescale; the geometric mean never exceeds
    // the arithmetic one, so the same 2^-k scale keeps it in [0,1]
    f2 pay = {clamp01(basket.x - o.strike), clamp01(basket.y - o.strike)};
    if (o.cv)  // wave-uniform
        pay -= (f2){clamp01(__builtin_amdgcn_exp2f(lg.x) - o.strike), clamp01(__builtin_amdgcn_exp2f(lg.y) - o.strike)};
    if (ANTI) {  // sum of the two values; the 1/2 rides on the finishing step's scale
        pay += (f2){clamp01(mirror.x - o.strike), clamp01(mirror.y - o.strike)};
        if (o.cv)
            pay -= (f2){clamp01(__builtin_amdgcn_exp2f(lgm.x) - o.strike), clamp01(__builtin_amdgcn_exp2f(lgm.y) - o.strike)};
    }
    return pay;
}

constexpr uint32_t BASKET_F32_FLUSH = 8;

template <int NA, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void basket_f32_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const BasketArgs<float, NA> o, const Work w, float *__restrict__ out,
                                                           float out_scale)
{
    const uint32_t stride = gridDim.x * GROUP;
    const uint32_t gtid = blockIdx.x * GROUP + threadIdx.x;
    const uint32_t full_trips = w.n_units / (2 * stride);  // trips in which every lane has both units
    double acc_s = 0.0, acc_q = 0.0;
    f2 s2 = {0.0f, 0.0f}, q2 = {0.0f, 0.0f};
    constexpr bool IN_LDS = basket_consts_in_lds<float, NA>();
    __shared__ float lds_consts[IN_LDS ? ConstsLds<float, NA>::COUNT : 1];
    if (IN_LDS)
        ConstsLds<float, NA>::stage(lds_consts, o);
    Gen gen(w);
    const auto pair = [&](uint32_t cA, uint32_t cB) __attribute__((always_inline)) {
        if constexpr (IN_LDS)
            return basket_pair_f32<NA, ANTI>(gen, o, ConstsLds<float, NA>{lds_consts}, w, cA, cB);
        else
            return basket_pair_f32<NA, ANTI>(gen, o, ConstsArg<float, NA>{o}, w, cA, cB);
    };
    uint32_t i = gtid;
    for (uint32_t trip = 0; trip < full_trips; ++trip, i += 2 * stride) {
        const f2 p = pair(w.unit_lo + i, w.unit_lo + i + stride);
        s2 += p;
        q2 = pk_fma(p, p, q2);
        if (out) {  // wave-uniform: per-path dump for the parity tests
            out[i] = p.x * out_scale;
            out[i + stride] = p.y * out_scale;
        }
        if ((trip & (BASKET_F32_FLUSH - 1)) == BASKET_F32_FLUSH - 1) {
            acc_s += (double)(s2.x + s2.y);
            acc_q += (double)(q2.x + q2.y);
            s2 = (f2){0.0f, 0.0f};
            q2 = (f2){0.0f, 0.0f};
        }
    }
    if (i < w.n_units) {  // the partial last trip: unit i, and unit i + stride where it exists
        const bool has_b = i + stride < w.n_units;
        f2 p = pair(w.unit_lo + i, w.unit_lo + (has_b ? i + stride : i));
        if (!has_b)
            p.y = 0.0f;
        s2 += p;
        q2 = pk_fma(p, p, q2);
        if (out) {
            out[i] = p.x * out_scale;
            if (has_b)
                out[i + stride] = p.y * out_scale;
        }
    }
    acc_s += (double)(s2.x + s2.y);
    acc_q += (double)(q2.x + q2.y);
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// ---- generic basket: runtime asset count beyond the compiled sizes (17 .. MC_MAX_ASSETS_GENERIC) ----
// The reference's N is any compile-time constant (MonteCarlo.h:16); sizes without a register-resident
// specialisation run here.  A lane's normals live in its own column of a dynamic-LDS array
// g[asset][lane] (consecutive lanes, consecutive addresses: conflict-free, and nobody else touches
// the column, so no barrier).  The triangular mat-vec is blocked 4 rows x 4 columns: one ds_read of
// g[b] feeds four rows' fmas (LDS traffic / 4), and the host lays the folded matrix out block-row by
// block-row, 4 row-values per column, zero-padded to whole blocks, so that each 4 x 4 tile is 16
// consecutive reals behind ONE wave-uniform (scalar) load.  Padded rows have coef = 0, padded columns
// multiply real normals by 0.  Same stream and estimator definitions as the specialised kernels.
template <class Real>
struct BasketDyn {
    const Real *consts;  // tiles (8 nb (nb + 1) reals, nb = ceil(n / 4)), then base[4 nb], coef[4 nb], wg[4 nb]
    int n;
    Real strike;
    Real cg;  // control variate constant (see BasketArgs)
    int cv;
};

template <class Real, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void basket_dyn_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const BasketDyn<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Real *g = reinterpret_cast<Real *>(lds_raw) + threadIdx.x;  // this lane's column, stride GROUP
    constexpr int NPB = Gen::template npb<Real>();
    const int nb = (o.n + 3) >> 2, np = nb * 4, nblk = (np + NPB - 1) / NPB;   // whole blocks: the column holds nblk * NPB normals
    // constant address space: wave-uniform reads become scalar loads (s_load_dwordx16 per tile) whatever the
    // compiler can or cannot prove about the kernel's global stores
    typedef const __attribute__((address_space(4))) Real *cptr;
    const cptr tiles = (cptr)o.consts, base = tiles + 8 * nb * (nb + 1), coef = base + np, wg = coef + np;
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        for (int b = 0; b < nblk; ++b) {
            Real z[NPB];
            gen.normals(w, w.unit_lo + i, (uint32_t)b, 2u /*MC_DOMAIN_BASKET*/, z);
#pragma unroll
            for (int j = 0; j < NPB; ++j)
                g[(b * NPB + j) * GROUP] = z[j];
        }
        Real basket = 0, mirror = 0, lg = o.cg, lgm = o.cg;
        cptr tile = tiles;
        for (int A = 0; A < nb; ++A) {
            Real x[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                x[r] = base[4 * A + r];
            for (int c4 = 0; c4 <= A; ++c4, tile += 16) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const Real gb = g[(4 * c4 + j) * GROUP];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        x[r] = fma_r(tile[4 * j + r], gb, x[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)   // wg is zero without the control variate: its sums are formed unconditionally
                basket_row<ANTI>(x[r], (Real)base[4 * A + r], (Real)coef[4 * A + r], [&] { return (Real)wg[4 * A + r]; }, 1, basket, mirror, lg, lgm);
        }
        const Real p = basket_sample<ANTI>(basket, mirror, lg, lgm, o.strike, o.cv);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// fp32 form of the generic kernel: TWO paths per lane (units i and i + stride), one in each half of a packed
// register pair, like basket_f32_kernel -- the uniforms' scaling, the radius scaling, z = r trig, every fma of
// the tiled mat-vec and the weighted sums issue as v_pk_*_f32, and each scalar-loaded tile value and each
// loop step serves two paths.  The lane's LDS column holds packed pairs (8 bytes per asset).
template <bool ANTI>
__global__ __launch_bounds__(GROUP) void basket_dyn_f32_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const BasketDyn<float> o, const Work w, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    f2 *g = reinterpret_cast<f2 *>(lds_raw) + threadIdx.x;  // this lane's column, stride GROUP
    const int nb = (o.n + 3) >> 2, np = nb * 4;             // nb Philox blocks (4 normals each) per path
    typedef const __attribute__((address_space(4))) float *cptr;
    const cptr tiles = (cptr)o.consts, base = tiles + 8 * nb * (nb + 1), coef = base + np, wg = coef + np;
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    GenPhilox gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += 2 * stride) {
        const bool has_b = i + stride < w.n_units;  // false only in a range's last trip
        const uint32_t cA = w.unit_lo + i, cB = w.unit_lo + (has_b ? i + stride : i);
        for (int b = 0; b < nb; ++b)
            basket_normals_pk<1>(gen, w, cA, cB, [&](int k) -> f2 & { return g[(4 * b + k) * GROUP]; }, (uint32_t)b);
        f2 basket = {0.0f, 0.0f}, mirror = {0.0f, 0.0f}, lg = bcast(o.cg), lgm = bcast(o.cg);
        cptr tile = tiles;
        for (int A = 0; A < nb; ++A) {
            f2 x[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                x[r] = bcast(base[4 * A + r]);
            for (int c4 = 0; c4 <= A; ++c4, tile += 16) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f2 gb = g[(4 * c4 + j) * GROUP];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        x[r] = pk_fma(bcast(tile[4 * j + r]), gb, x[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                basket_row_pk<ANTI>(x[r], base[4 * A + r], coef[4 * A + r], [&] { return wg[4 * A + r]; }, 1, basket, mirror, lg, lgm);
        }
        f2 p = basket_sample_pk<ANTI>(basket, mirror, lg, lgm, o.strike, o.cv);
        if (!has_b)
            p.y = 0.0f;
        acc_s += (double)p.x + (double)p.y;
        acc_q = __builtin_fma((double)p.x, (double)p.x, __builtin_fma((double)p.y, (double)p.y, acc_q));
        if (out) {
            out[i] = p.x;
            if (has_b)
                out[i + stride] = p.y;
        }
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// ---- tiled basket with register-resident normals: the larger fp64 sizes -----------------------
// Same constant buffer and tile layout as the generic kernel, but the asset count is bounded at compile
// time, the normals stay in registers and everything is unrolled (padding rows, columns and the zeros
// above the diagonal are skipped at compile time).  The folded matrix never sits in
// registers across a trip: each half tile (4 rows x 2 columns = 8 reals) is one scalar load from constant
// memory issued one half tile ahead of its use, so the constants cost no VALU slot (the SGPR path pays a
// v_readlane_b32 per use once they no longer fit: 329 of 1457 instructions at n=16) and no LDS latency.
// What keeps hipcc from hoisting these loop-invariant loads out of the path loop (and spilling them again)
// is an offset it cannot see through: an empty volatile asm that redefines `off` (always 0) and is tied
// to the value computed just before, which also fixes where in the trip each load is issued.
// A wave-uniform value (in an SGPR pair) into a vector register pair with ONE v_mov_b64 (hipcc emits two v_mov_b32).
__device__ __forceinline__ double scalar_to_vgpr(double x)
{
    double r;
    asm("v_mov_b64 %0, %1" : "=v"(r) : "s"(x));
    return r;
}
__device__ __forceinline__ float scalar_to_vgpr(float x) { return x; }

template <class Real, int NA, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void basket_tiled_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const BasketDyn<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    constexpr int NB = (NA + 3) / 4, NP = 4 * NB, NPB = Gen::template npb<Real>(), NBLK = (NA + NPB - 1) / NPB;
    constexpr int NH = NB * (NB + 1);  // half tiles in the buffer
    typedef const __attribute__((address_space(4))) Real *cptr;
    const cptr tiles = (cptr)o.consts, base = tiles + 8 * NH, coef = base + NP, wg = coef + NP;
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        Real g[NBLK * NPB];
        basket_normals(gen, w, w.unit_lo + i, g);
        Real basket = 0, mirror = 0, lg = o.cg, lgm = o.cg;
        Real tl[2][8];
        int off = 0;
        asm volatile("" : "+s"(off) : "v"(g[0]));
#pragma unroll
        for (int k = 0; k < 8; ++k)
            tl[0][k] = tiles[off + k];
        int slot = 0;  // which of the two register tiles holds the half tile in use (compile-time after unrolling)
#pragma unroll
        for (int A = 0; A < NB; ++A) {
            constexpr int ROWS_LAST = NA - 4 * (NB - 1);
            const int rows = A == NB - 1 ? ROWS_LAST : 4;   // rows of this block row that exist
            const int halves = (4 * A + rows + 1) / 2;      // half tiles that hold a column <= the last row's diagonal
            Real x[4], cf[4], wr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r < rows) {
                    x[r] = scalar_to_vgpr(base[off + 4 * A + r]);
                    cf[r] = coef[off + 4 * A + r];
                    wr[r] = wg[off + 4 * A + r];
                }
#pragma unroll
            for (int c2 = 0; c2 < 2 * (A + 1); ++c2) {
                if (c2 >= halves)
                    continue;
                // the half tile used next: the following one of this block row, or the first of the next block row
                const int h = A * (A + 1) + c2;
                const int h_next = c2 + 1 < halves ? h + 1 : (A + 1 < NB ? (A + 1) * (A + 2) : -1);
                if (h_next >= 0) {  // issued now, used after this half tile's fmas
                    asm volatile("" : "+s"(off) : "v"(x[0]));
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        tl[slot ^ 1][k] = tiles[off + 8 * h_next + k];
                }
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (r < rows && 2 * c2 + j <= 4 * A + r)   // inside the lower triangle
                            x[r] = fma_r(tl[slot][4 * j + r], g[2 * c2 + j], x[r]);
                slot ^= 1;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r < rows)
                    basket_row<ANTI>(x[r], (Real)base[off + 4 * A + r], cf[r], [&] { return wr[r]; }, 1, basket, mirror, lg, lgm);
        }
        const Real p = basket_sample<ANTI>(basket, mirror, lg, lgm, o.strike, o.cv);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// fp32 form of the tiled kernel (12..32 assets): two paths per lane in packed halves (like basket_f32_kernel
// and basket_dyn_f32_kernel), normals in registers, each whole 4 x 4 tile (16 floats) one scalar load issued a
// tile ahead.  Plain max for the payoff (no power-of-two rescale: the host folds none for these sizes).
template <int NA, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void basket_tiled_f32_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const BasketDyn<float> o, const Work w, float *__restrict__ out)
{
    constexpr int NB = (NA + 3) / 4, NP = 4 * NB, NT = NB * (NB + 1) / 2;
    typedef const __attribute__((address_space(4))) float *cptr;
    const cptr tiles = (cptr)o.consts, base = tiles + 16 * NT, coef = base + NP, wg = coef + NP;
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += 2 * stride) {
        const bool has_b = i + stride < w.n_units;  // false only in a range's last trip
        const uint32_t cA = w.unit_lo + i, cB = w.unit_lo + (has_b ? i + stride : i);
        f2 g[NP];
        basket_normals_pk<NB>(gen, w, cA, cB, [&](int k) -> f2 & { return g[k]; });
        f2 basket = {0.0f, 0.0f}, mirror = {0.0f, 0.0f}, lg = bcast(o.cg), lgm = bcast(o.cg);
        float tl[2][16];
        int off = 0;
        asm volatile("" : "+s"(off) : "v"(g[0].x));
#pragma unroll
        for (int k = 0; k < 16; ++k)
            tl[0][k] = tiles[off + k];
        int t = 0;  // tile counter (compile-time after unrolling)
#pragma unroll
        for (int A = 0; A < NB; ++A) {
            constexpr int ROWS_LAST = NA - 4 * (NB - 1);
            const int rows = A == NB - 1 ? ROWS_LAST : 4;  // rows of this block row that exist
            f2 x[4];
            float cf[4], wr[4], bs[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r < rows) {
                    bs[r] = base[off + 4 * A + r];
                    cf[r] = coef[off + 4 * A + r];
                    wr[r] = wg[off + 4 * A + r];
                    x[r] = bcast(bs[r]);
                }
#pragma unroll
            for (int c4 = 0; c4 <= A; ++c4, ++t) {
                if (t + 1 < NT) {  // next tile: issued now, used after this one's fmas
                    asm volatile("" : "+s"(off) : "v"(x[0].x));
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        tl[(t + 1) & 1][k] = tiles[off + 16 * (t + 1) + k];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (r < rows && 4 * c4 + j <= 4 * A + r)   // an existing row, inside the lower triangle
                            x[r] = pk_fma(bcast(tl[t & 1][4 * j + r]), g[4 * c4 + j], x[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r < rows)
                    basket_row_pk<ANTI>(x[r], bs[r], cf[r], [&] { return wr[r]; }, 1, basket, mirror, lg, lgm);
        }
        f2 p = basket_sample_pk<ANTI>(basket, mirror, lg, lgm, o.strike, o.cv);
        if (!has_b)
            p.y = 0.0f;
        acc_s += (double)p.x + (double)p.y;
        acc_q = __builtin_fma((double)p.x, (double)p.x, __builtin_fma((double)p.y, (double)p.y, acc_q));
        if (out) {
            out[i] = p.x;
            if (has_b)
                out[i + stride] = p.y;
        }
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// ---- 16-asset fp64 basket with the correlation step on the matrix cores ------------------------
// The Cholesky step x = base + M g of 64 paths is a 16 x 16 by 16 x 64 product (BASELINE.json north_star: "MFMA only if
// the basket Cholesky step is cast as a dense small-matrix contraction"): four column blocks of 16 paths, each
// 4 x v_mfma_f64_16x16x4_f64, take the 136 v_fma_f64 per path of the mat-vec out of the vector pipe, which is what the
// kernel is bound by.  No transposition through LDS: Philox is counter-based, so a lane simply
// generates the normals the B operand wants from it.  Lane l = 16 q + j holds, for column block c (paths i0 + 16 c + j),
// the normals of Philox blocks q and q + 4 of that path, i.e. columns k(s, q) = 2 q, 2 q + 1, 2 q + 8, 2 q + 9 of M for
// the k-steps s = 0..3 -- the host lays M out as the A operand of each step in exactly that column order (BasketDyn
// consts, after wg: a4[s][lane] = M[j][k(s, q)]).  A lane does the same RNG work as before (8 blocks, 16 normals per
// trip), for 4 paths x 4 columns instead of 1 path x 16.
// The accumulators come back as X[asset q + 4 v][path i0 + 16 c + j], v = 0..3: 16 exponentials per lane as before,
// the weighted sum over assets is 4 in-lane fmas per column block plus a sum over the four lane groups, done as a
// reduce-scatter with v_permlane32_swap / v_permlane16_swap (6 swaps + 3 adds) that leaves lane l with the basket of
// path i0 + l: units, per-lane sums and the closing reduction are those of every other basket kernel.
// Differences from them: the order of the additions inside x and inside the basket sum (results agree to a few ulp,
// not bit for bit), and a wave prices all 64 paths of a trip or none (paths beyond the range are computed and dropped).
typedef double d4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// a's lanes 32..63 <-> b's lanes 0..31
__device__ __forceinline__ void swap_halves(double &a, double &b)
{
    uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
    const u32x2 lo = __builtin_amdgcn_permlane32_swap((uint32_t)ua, (uint32_t)ub, false, false);
    const u32x2 hi = __builtin_amdgcn_permlane32_swap((uint32_t)(ua >> 32), (uint32_t)(ub >> 32), false, false);
    a = __builtin_bit_cast(double, (uint64_t)lo.x | ((uint64_t)hi.x << 32));
    b = __builtin_bit_cast(double, (uint64_t)lo.y | ((uint64_t)hi.y << 32));
}
// a's odd rows of 16 lanes <-> b's even rows
__device__ __forceinline__ void swap_rows(double &a, double &b)
{
    uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
    const u32x2 lo = __builtin_amdgcn_permlane16_swap((uint32_t)ua, (uint32_t)ub, false, false);
    const u32x2 hi = __builtin_amdgcn_permlane16_swap((uint32_t)(ua >> 32), (uint32_t)(ub >> 32), false, false);
    a = __builtin_bit_cast(double, (uint64_t)lo.x | ((uint64_t)hi.x << 32));
    b = __builtin_bit_cast(double, (uint64_t)lo.y | ((uint64_t)hi.y << 32));
}
// p[c] = lane group q's share of the sum for path block c; returns the whole sum for path block q (this lane's own path)
__device__ __forceinline__ double sum_over_lane_groups(double p0, double p1, double p2, double p3)
{
    swap_halves(p0, p2);   // lower half keeps c = 0, upper half c = 2
    swap_halves(p1, p3);   //                  c = 1             c = 3
    double r0 = p0 + p2, r1 = p1 + p3;
    swap_rows(r0, r1);     // even rows keep r0's block, odd rows r1's
    return r0 + r1;
}

// Pair q (a lane-dependent 0..3) of fp64 block `block` of a path: words W[3q .. 3q + 2] of the block's twelve
// (mc_rng.hpp: words_to_normals).  They sit in Philox blocks 3 block + {0,0,1,2}[q] and 3 block + {0,1,2,2}[q]: two
// Philox blocks per pair here (the other kernels, which use all four pairs of a lane's block, pay three per four pairs) --
// one more reason this variant is not the default.
__device__ __forceinline__ void mfma_pair_normals(GenPhilox &gen, const Work &w, uint32_t unit, uint32_t block, int q, double (&z)[2])
{
    const uint32_t ba = (3u * (uint32_t)q) >> 2, bb = (3u * (uint32_t)q + 2u) >> 2;
    const u32x4 ra = gen.words(w, unit, 3u * block + ba, 2u /*MC_DOMAIN_BASKET*/);
    const u32x4 rb = gen.words(w, unit, 3u * block + bb, 2u);
    const uint32_t a = q == 0 ? ra.x : (q == 1 ? ra.w : (q == 2 ? ra.z : ra.y));   // W[3q]
    const uint32_t m = q == 0 ? ra.y : (q == 1 ? rb.x : (q == 2 ? ra.w : ra.z));   // W[3q + 1]
    const uint32_t c = q == 0 ? ra.z : (q == 1 ? rb.y : (q == 2 ? rb.x : rb.w));   // W[3q + 2]
    pair_normals_f64(a, m, c, z[0], z[1]);
}

template <bool ANTI>
__global__ __launch_bounds__(GROUP) void basket_mfma_f64_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const BasketDyn<double> o, const Work w, double *__restrict__ out)
{
    stage_tables<double>();
    constexpr int NB = 4, NP = 16, NH = NB * (NB + 1);
    const double *base = o.consts + 8 * NH, *coef = base + NP, *wg = coef + NP, *a4 = wg + NP;
    const int lane = threadIdx.x & 63, q = lane >> 4, j = lane & 15;
    double A[4], cb[4], cf[4], wr[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        A[s] = a4[64 * s + lane];
        cb[s] = base[q + 4 * s];
        cf[s] = coef[q + 4 * s];
        wr[s] = wg[q + 4 * s];
    }
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    GenPhilox gen(w);
    // wave-uniform trip count: the matrix instructions want all 64 lanes
    for (uint32_t i0 = blockIdx.x * GROUP + (threadIdx.x & ~63u); i0 < w.n_units; i0 += stride) {
        double pb[4], pm[4], pl[4], plm[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t unit = w.unit_lo + i0 + 16u * c + j;
            double za[2], zb[2];
            mfma_pair_normals(gen, w, unit, 0u, q, za);   // columns 2q, 2q + 1:     pair q of the path's first fp64 block
            mfma_pair_normals(gen, w, unit, 1u, q, zb);   // columns 2q + 8, 2q + 9: pair q of its second
            d4 x = {cb[0], cb[1], cb[2], cb[3]};
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(A[0], za[0], x, 0, 0, 0);
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(A[1], za[1], x, 0, 0, 0);
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(A[2], zb[0], x, 0, 0, 0);
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(A[3], zb[1], x, 0, 0, 0);
            double b = 0, m = 0, l = 0, lm = 0;
#pragma unroll
            for (int v = 0; v < 4; ++v)
                basket_row<ANTI>(x[v], cb[v], cf[v], [&] { return wr[v]; }, 1, b, m, l, lm);
            pb[c] = b, pm[c] = m, pl[c] = l, plm[c] = lm;
        }
        // the sums over the four lane groups (the control variate's only when it is on: wave-uniform)
        const double basket = sum_over_lane_groups(pb[0], pb[1], pb[2], pb[3]);
        const double mirror = ANTI ? sum_over_lane_groups(pm[0], pm[1], pm[2], pm[3]) : 0.0;
        const double lg = o.cv ? o.cg + sum_over_lane_groups(pl[0], pl[1], pl[2], pl[3]) : 0.0;
        const double lgm = (ANTI && o.cv) ? o.cg + sum_over_lane_groups(plm[0], plm[1], plm[2], plm[3]) : 0.0;
        double p = basket_sample<ANTI>(basket, mirror, lg, lgm, o.strike, o.cv);
        const uint32_t i = i0 + lane;
        if (i >= w.n_units)
            p = 0;
        acc_s += p;
        acc_q = __builtin_fma(p, p, acc_q);
        if (out && i < w.n_units)
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// CVA of one call.  Reference device loop, dp/MonteCarloKernel.cu:241-262 (spot advanced
// first, exposure = Black-Scholes value at the NEW spot and residual maturity :125-129, with
// the Hastings CDF :110-123).  Everything that depends only on the date j is tabulated once
// per call on the host in fp64 (the reference recomputes it per path per step, :248):
//   W_j = z_1 + ... + z_j                       (the lane's only state)
//   d1 = W_j g_j + e1_j,  d2 = W_j g_j + e2_j   g_j = v sqrt(dt) / (v sqrt(tau_j))
//   s_j = E(W_j bx + xk_j)                      ln s_j = ln S0 + j a + v sqrt(dt) W_j
//   ee_j = s_j cnd(d1) - disc_j cnd(d2)         disc_j = K exp(-r tau_j)
//   cva  = LGD * sum_j dp_j ee_j
// A final date with residual maturity exactly 0 uses the intrinsic value.
// =========================================================================================
template <class Real>
struct CvaStep {
    Real g, e1, e2, xk, disc, dp;
};
template <class Real>
struct CvaArgs {
    const CvaStep<Real> *steps;  // n_bs Black-Scholes dates (+1 intrinsic date if last_intrinsic)
    const float *pairs;          // fp32 only: the same rows for date pairs (2q, 2q + 1), field by field:
                                 // {g, g', e1, e1', e2, e2', xk, xk', disc, disc', dp, dp'}, floor(n_bs / 2) pairs
    int n_bs;                    // dates priced with the closed form
    int last_intrinsic;          // 1: one more date, residual maturity == 0
    Real bx;                     // v sqrt(dt) (times log2 e in f32)
    Real lgd, strike;
    const Real *extra;           // Greeks only: sqrt(tau_j) for every date, then sigma t_j for every date (2 (n_bs + last_intrinsic) reals)
    int pairs_in_lds;            // fp32 one-lane-per-path loop: the launch carries dynamic LDS for `pairs` (host: cva_enqueue), rows come as ds_read_b128
};

// Black-Scholes exposure at one date, from the lane's state W and the date's table row.
// Reference: device_bsCall + cnd, dp/MonteCarloKernel.cu:110-129.  With T(d) = phi(d) P(1/(1+c|d|))
// (Hastings 26.2.17, same constants) cnd(d) = d > 0 ? 1 - T(d) : T(d), and the Black-Scholes
// identity  S phi(d1) = K e^{-r tau} phi(d2)  lets ONE exponential serve both terms:
//     A = S phi(d1) = C exp(ln S - d1^2 / 2)
//     S cnd(d1) = d1 > 0 ? S - A P1 : A P1,      K e^{-r tau} cnd(d2) = d2 > 0 ? disc - A P2 : A P2
// -- evaluated without the selects by signed_tails below --
// (the reference evaluates three exponentials per date here: :106,:118 twice,:128).
// ln S is the value the spot's own exponential is taken of, so A costs one fma + one exponential.
// S cnd(d1) - K' cnd(d2) from the two upper tails t1 = S tail(|d1|), t2 = K' tail(|d2|), without selects:
//     cnd(d) = 1/2 + sgn(d) (1/2 - tail(|d|))   =>   (S - K')/2 + sgn(d1) (S/2 - t1) - sgn(d2) (K'/2 - t2)
// sgn(d) x is x with d's sign bit xor-ed into its (high) word: ONE v_bitop3_b32 (a ^ (b & c), truth table 0x78).
// fp64: 7 instructions per date instead of 9 (two subtractions, two compares, four v_cndmask, one subtraction): -1.3 ... -2.4 %
// kernel time on the 256-date CVA, in-process (profiles/r03_ab_cva_signed_tails.log); same bits as the select form up to
// the roundings of S/2 - t (per-path difference from the oracle unchanged: 1.5e-14 against 1.4e-14).
__device__ __forceinline__ float flip_by_sign(float x, float d)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_bitop3_b32(__builtin_bit_cast(uint32_t, x), __builtin_bit_cast(uint32_t, d), 0x80000000u, 0x78));
}
__device__ __forceinline__ double flip_by_sign(double x, double d)
{
    return __hiloint2double((int)__builtin_amdgcn_bitop3_b32((uint32_t)__double2hiint(x), (uint32_t)__double2hiint(d), 0x80000000u, 0x78),
                            __double2loint(x));
}
template <class Real>
__device__ __forceinline__ Real signed_tails(Real spot, Real disc, Real d1, Real d2, Real t1, Real t2)
{
    const Real w1 = flip_by_sign(fma_r((Real)0.5, spot, -t1), d1);
    const Real w2 = flip_by_sign(fma_r((Real)0.5, disc, -t2), d2);
    return fma_r((Real)0.5, spot - disc, w1 - w2);
}

__device__ __forceinline__ float bs_exposure(float ln2_spot, float W, const CvaStep<float> &st)
{
    const float spot = __builtin_amdgcn_exp2f(ln2_spot);
    // d1, d2 and everything downstream as one packed pair
    const f2 d = __builtin_elementwise_fma((f2){W, W}, (f2){st.g, st.g}, (f2){st.e1, st.e2});
    const float A = 0.3989422804014327f * __builtin_amdgcn_exp2f(__builtin_fmaf(d.x * -0.72134752044448170f, d.x, ln2_spot));
    const f2 den = __builtin_elementwise_fma((f2){0.2316419f, 0.2316419f}, __builtin_elementwise_abs(d), (f2){1.0f, 1.0f});
    const f2 k = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
    f2 poly = __builtin_elementwise_fma(k, (f2){1.330274429f, 1.330274429f}, (f2){-1.821255978f, -1.821255978f});
    poly = __builtin_elementwise_fma(k, poly, (f2){1.781477937f, 1.781477937f});
    poly = __builtin_elementwise_fma(k, poly, (f2){-0.356563782f, -0.356563782f});
    poly = __builtin_elementwise_fma(k, poly, (f2){0.31938153f, 0.31938153f});
    const f2 t = poly * k * (f2){A, A};
    return signed_tails(spot, st.disc, d.x, d.y, t.x, t.y);
}

// fp32, TWO consecutive dates of one path in the halves of every packed op (the form above packs d1, d2 of one
// date): the same operations per date, but the spot's exponent, A, the selects' subtractions and the dp-weighted
// accumulation now issue packed as well.  `row` = 12 floats {g, e1, e2, xk, disc, dp} x {date, next date}.
__device__ __forceinline__ f2 bs_exposure_dates(f2 ln2_spot, f2 W, f2 g, f2 e1, f2 e2, f2 disc)
{
    const f2 spot = {__builtin_amdgcn_exp2f(ln2_spot.x), __builtin_amdgcn_exp2f(ln2_spot.y)};
    const f2 d1 = __builtin_elementwise_fma(W, g, e1), d2 = __builtin_elementwise_fma(W, g, e2);
    const f2 a = __builtin_elementwise_fma(d1 * (f2){-0.72134752044448170f, -0.72134752044448170f}, d1, ln2_spot);
    const f2 A = (f2){0.3989422804014327f, 0.3989422804014327f} * (f2){__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
    const f2 c = {0.2316419f, 0.2316419f}, one = {1.0f, 1.0f};
    const f2 den1 = __builtin_elementwise_fma(c, __builtin_elementwise_abs(d1), one);
    const f2 den2 = __builtin_elementwise_fma(c, __builtin_elementwise_abs(d2), one);
    const f2 k1 = {__builtin_amdgcn_rcpf(den1.x), __builtin_amdgcn_rcpf(den1.y)};
    const f2 k2 = {__builtin_amdgcn_rcpf(den2.x), __builtin_amdgcn_rcpf(den2.y)};
    const f2 c4 = {1.330274429f, 1.330274429f}, c3 = {-1.821255978f, -1.821255978f}, c2 = {1.781477937f, 1.781477937f},
             c1 = {-0.356563782f, -0.356563782f}, c0 = {0.31938153f, 0.31938153f};
    f2 p1 = __builtin_elementwise_fma(k1, c4, c3), p2 = __builtin_elementwise_fma(k2, c4, c3);
    p1 = __builtin_elementwise_fma(k1, p1, c2);
    p2 = __builtin_elementwise_fma(k2, p2, c2);
    p1 = __builtin_elementwise_fma(k1, p1, c1);
    p2 = __builtin_elementwise_fma(k2, p2, c1);
    p1 = __builtin_elementwise_fma(k1, p1, c0);
    p2 = __builtin_elementwise_fma(k2, p2, c0);
    const f2 t1 = p1 * k1 * A, t2 = p2 * k2 * A;
    // signed_tails, both dates packed: the sign flips are the only per-lane instructions
    const f2 half = {0.5f, 0.5f};
    const f2 v1 = __builtin_elementwise_fma(half, spot, -t1), v2 = __builtin_elementwise_fma(half, disc, -t2);
    const f2 w1 = {flip_by_sign(v1.x, d1.x), flip_by_sign(v1.y, d1.y)}, w2 = {flip_by_sign(v2.x, d2.x), flip_by_sign(v2.y, d2.y)};
    return __builtin_elementwise_fma(half, spot - disc, w1 - w2);
}
__device__ __forceinline__ f2 bs_exposure_dates(f2 ln2_spot, f2 W, const float *row)
{
    return bs_exposure_dates(ln2_spot, W, (f2){row[0], row[1]}, (f2){row[2], row[3]}, (f2){row[4], row[5]}, (f2){row[8], row[9]});
}

// a * b + c with c read from its SGPR pair by the three-operand instruction (c must be wave-uniform)
__device__ __forceinline__ double fma_scalar_addend(double a, double b, double c)
{
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}
// a wave-uniform value in a vector register pair (one copy, where hipcc would make one per use)
__device__ __forceinline__ double to_vgpr(double x)
{
    asm("" : "+v"(x));
    return x;
}

__device__ __forceinline__ double hastings_poly(double k)
{
    double poly = __builtin_fma(k, 1.330274429, -1.821255978);
    poly = __builtin_fma(k, poly, 1.781477937);
    poly = __builtin_fma(k, poly, -0.356563782);
    poly = __builtin_fma(k, poly, 0.31938153);
    return poly * k;
}

// the same polynomial times 1/sqrt(2 pi): coefficients pre-multiplied (each rounded once, at compile time)
__device__ __forceinline__ double hastings_poly_phi(double k)
{
    constexpr double C = 0.39894228040143267793994605993438;
    double poly = __builtin_fma(k, C * 1.330274429, C * -1.821255978);
    poly = __builtin_fma(k, poly, C * 1.781477937);
    poly = __builtin_fma(k, poly, C * -0.356563782);
    poly = __builtin_fma(k, poly, C * 0.31938153);
    return poly * k;
}

__device__ __forceinline__ double bs_exposure(double ln_spot, double W, const CvaStep<double> &st)
{
    const double spot = exp_f64(ln_spot);
    const double d1 = __builtin_fma(W, st.g, st.e1), d2 = __builtin_fma(W, st.g, st.e2);
    const double A = 0.39894228040143267793994605993438 * exp_f64(fmax(__builtin_fma(-0.5 * d1, d1, ln_spot), -800.0));  // d1 runs away as tau -> 0
    double k1, k2;
    recip2_pos(__builtin_fma(0.2316419, fabs(d1), 1.0), __builtin_fma(0.2316419, fabs(d2), 1.0), k1, k2);
    const double t1 = A * hastings_poly(k1);
    const double t2 = A * hastings_poly(k2);
    return signed_tails(spot, st.disc, d1, d2, t1, t2);
}

// fp64: two consecutive dates of a path together, so that their four Hastings reciprocals share one v_rcp_f64 (a
// 16-cycle instruction: -3.7 % kernel time for sharing in pairs, a further -1.3 % for four).  Same operations per date
// as bs_exposure except for that shared reciprocal and 1/sqrt(2 pi) folded into the Hastings coefficients.
template <bool SGPR_ROWS = true>
__device__ __forceinline__ void bs_exposure2(double ln_a, double W_a, const CvaStep<double> &sa, double ln_b, double W_b,
                                             const CvaStep<double> &sb, double &ee_a, double &ee_b)
{
    const double spot_a = exp_f64(ln_a), spot_b = exp_f64(ln_b);
    // The table row sits in SGPRs and a VALU instruction reads at most one scalar operand.  hipcc turns fma(W, g, e)
    // with g and e both scalar into v_fmac_f64 and copies the ADDEND into the destination pair first (two v_mov_b32 per
    // fma: 6 of the ~124 instructions per date).  Spelled out instead: g into a vector pair once (it serves d1 and d2),
    // the addends read straight from their SGPRs by the three-operand form -- same fma, same bits, 3 instructions per
    // date instead of 6 (-3.1 % instructions, -2.4 % time: profiles/r02_ab_cva_scalar_addend.log).
    // (SGPR_ROWS = false: the date differs between lanes -- cva_dates_kernel -- and the rows are ordinary vector operands)
    double d1a, d2a, d1b, d2b;
    if constexpr (SGPR_ROWS) {
        const double g_a = scalar_to_vgpr(sa.g), g_b = scalar_to_vgpr(sb.g);
        d1a = fma_scalar_addend(W_a, g_a, sa.e1), d2a = fma_scalar_addend(W_a, g_a, sa.e2);
        d1b = fma_scalar_addend(W_b, g_b, sb.e1), d2b = fma_scalar_addend(W_b, g_b, sb.e2);
    } else {
        d1a = __builtin_fma(W_a, sa.g, sa.e1), d2a = __builtin_fma(W_a, sa.g, sa.e2);
        d1b = __builtin_fma(W_b, sb.g, sb.e1), d2b = __builtin_fma(W_b, sb.g, sb.e2);
    }
    // A = C exp(.) with C = 1/sqrt(2 pi) folded into the Hastings coefficients (hastings_poly_phi): one multiply less per date
    const double A_a = exp_f64(fmax(__builtin_fma(-0.5 * d1a, d1a, ln_a), -800.0));  // d1 runs away as tau -> 0
    const double A_b = exp_f64(fmax(__builtin_fma(-0.5 * d1b, d1b, ln_b), -800.0));
    double k1a, k2a, k1b, k2b;
    recip4_pos(__builtin_fma(0.2316419, fabs(d1a), 1.0), __builtin_fma(0.2316419, fabs(d2a), 1.0),
               __builtin_fma(0.2316419, fabs(d1b), 1.0), __builtin_fma(0.2316419, fabs(d2b), 1.0), k1a, k2a, k1b, k2b);
    const double t1a = A_a * hastings_poly_phi(k1a), t2a = A_a * hastings_poly_phi(k2a);
    const double t1b = A_b * hastings_poly_phi(k1b), t2b = A_b * hastings_poly_phi(k2b);
    ee_a = signed_tails(spot_a, sa.disc, d1a, d2a, t1a, t2a);
    ee_b = signed_tails(spot_b, sb.disc, d1b, d2b, t1b, t2b);
}

// One date the slow way: any date of a block that the pair forms below do not cover (a block's tail at the end of the
// grid, the intrinsic-value date).  j is wave-uniform: the table row comes through scalar loads.
template <class Real, bool ANTI>
__device__ __forceinline__ void cva_single_date(const CvaArgs<Real> &o, int j, int n_dates, Real z, Real &W, Real &acc)
{
    if (j >= n_dates)
        return;
    const CvaStep<Real> st = o.steps[j];
    W += z;
    const Real ln_spot = fma_r(W, o.bx, st.xk);     // natural log in f64, log2 in f32
    const Real ln_mirror = fma_r(-W, o.bx, st.xk);  // the path driven by -z (ANTI only)
    Real ee;
    if (j < o.n_bs) {
        ee = bs_exposure(ln_spot, W, st);
        if (ANTI)
            ee += bs_exposure(ln_mirror, -W, st);
    } else {
        const Real iv = exp_model(ln_spot) - o.strike;
        ee = iv > 0 ? iv : 0;
        if (ANTI) {
            const Real ivm = exp_model(ln_mirror) - o.strike;
            ee += ivm > 0 ? ivm : 0;
        }
    }
    acc = fma_r(st.dp, ee, acc);
}

// fp32: a block of four normals = two packed date pairs per trip of the date loop.
__device__ __forceinline__ f2 exposure_pair_rows(float bx, f2 Wp, const float (&row)[12]);   // below, next to the date-parallel role that shares it
// `lds_pairs`: the workgroup's LDS copy of o.pairs, or nullptr.  From scalar registers a pair's row costs six v_mov_b32 per pair (a
// packed fma takes ONE scalar operand, so every addend and second factor is copied into vector registers first: 12 of the 169
// instructions per four dates); from LDS the twelve floats arrive in vector registers as three ds_read_b128 at a wave-uniform
// address, which issue beside the VALU (44 instead of 49 vector instructions per pair; -2.5 % at 19 trips, -2.3 % at 1e7 paths in one
// process: profiles/r06_ab_cva_f32_rows_in_lds.log).  Same operations on the same values either way.
template <bool ANTI, class Gen>
__device__ __forceinline__ float cva_path(Gen &gen, const CvaArgs<float> &o, const Work &w, uint32_t c0, const float *lds_pairs = nullptr)
{
    constexpr int NPB = Gen::template npb<float>();
    static_assert(NPB == 4, "two packed date pairs per block");
    float W = 0, acc = 0;
    f2 acc2 = {0.0f, 0.0f};  // even / odd dates of the packed date pairs
    float z[NPB];
    const int n_dates = o.n_bs + o.last_intrinsic;
    for (int j0 = 0; j0 < n_dates; j0 += NPB) {
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 3u /*MC_DOMAIN_CVA*/, z);
#pragma unroll
        for (int h = 0; h < NPB / 2; ++h) {
            const int j = j0 + 2 * h;
            if (j + 1 < o.n_bs) {  // wave-uniform: both dates of this pair have a closed-form exposure
                // the pair's rows once more, field by field ({g, g'} ... {dp, dp'} adjacent: mc_api.hip), so the two dates
                // ride in the halves of every packed instruction (-8 % against packing d1, d2 of one date)
                const f2 Wp = {W + z[2 * h], (W + z[2 * h]) + z[2 * h + 1]};
                W = Wp.y;
                if (lds_pairs) {   // wave-uniform
                    float row[12];
                    const float4 *src = reinterpret_cast<const float4 *>(lds_pairs + 12 * (j / 2));
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const float4 v = src[q];
                        row[4 * q] = v.x, row[4 * q + 1] = v.y, row[4 * q + 2] = v.z, row[4 * q + 3] = v.w;
                    }
                    f2 ee = exposure_pair_rows(o.bx, Wp, row);
                    if (ANTI)
                        ee += exposure_pair_rows(o.bx, -Wp, row);
                    acc2 = pk_fma((f2){row[10], row[11]}, ee, acc2);
                } else {
                    const float *row = o.pairs + 12 * (j / 2);
                    const f2 bx = {o.bx, o.bx}, xk = {row[6], row[7]}, dp = {row[10], row[11]};
                    f2 ee = bs_exposure_dates(pk_fma(Wp, bx, xk), Wp, row);
                    if (ANTI)
                        ee += bs_exposure_dates(pk_fma(-Wp, bx, xk), -Wp, row);
                    acc2 = pk_fma(dp, ee, acc2);
                }
            } else {
                cva_single_date<float, ANTI>(o, j, n_dates, z[2 * h], W, acc);
                cva_single_date<float, ANTI>(o, j + 1, n_dates, z[2 * h + 1], W, acc);
            }
        }
    }
    acc += acc2.x + acc2.y;
    return acc * (ANTI ? o.lgd * 0.5f : o.lgd);
}

// fp64: dates in Box-Muller pairs drawn through the generator's pair cursor (mc_rng.hpp): the fp64 stream hands out eight
// normals per block, and a date loop that draws all eight at once keeps four pairs of table rows in SGPRs (they spill into
// VGPR lanes) and eight normals in VGPRs.  The cursor draws one pair at a time; the loop runs FOUR pairs per trip with the
// cursor's phase a compile-time constant in each copy (round 6: 793 vector instructions per eight dates instead of 4 x 216,
// -3.4 % at C5's shard and -4.2 % at C5 in one process, profiles/r06_ab_cva_four_pairs.log; 129 VGPRs = 3 waves per SIMD,
// and forcing 4 with amdgpu_waves_per_eu changes nothing), and one pair per trip for what is left of the grid.
template <bool ANTI, class Gen>
__device__ __forceinline__ double cva_path(Gen &gen, const CvaArgs<double> &o, const Work &w, uint32_t c0)
{
    double W = 0, acc = 0;
    const int n_dates = o.n_bs + o.last_intrinsic;
    const double bx_v = to_vgpr(o.bx);   // in a vector register for the whole path: ln s = fma(W, bx, xk_j) then reads ONE scalar (xk_j)
    // the polynomial coefficients of the pair's Box-Muller as opaque vector registers: one three-operand v_fma_f64 per Horner step
    // instead of hipcc's v_mov + v_fmac (mc_math_f64.hpp: F64K; 9 of the 225 instructions per two dates -- the exponentials and
    // Hastings tails of the exposure gain nothing from the same treatment and stay on literals)
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    // dates j, j + 1 (both with a closed-form exposure) from one pair of normals
    auto closed_pair = [&](int j, double z0, double z1) {
        const CvaStep<double> sa = o.steps[j], sb = o.steps[j + 1];
        const double W_a = W + z0, W_b = W_a + z1;
        W = W_b;
        double ee_a, ee_b;
        bs_exposure2(fma_scalar_addend(W_a, bx_v, sa.xk), W_a, sa, fma_scalar_addend(W_b, bx_v, sb.xk), W_b, sb, ee_a, ee_b);
        if (ANTI) {
            double em_a, em_b;
            bs_exposure2(fma_scalar_addend(-W_a, bx_v, sa.xk), -W_a, sa, fma_scalar_addend(-W_b, bx_v, sb.xk), -W_b, sb, em_a, em_b);
            ee_a += em_a;
            ee_b += em_b;
        }
        acc = fma_r(sa.dp, ee_a, acc);
        acc = fma_r(sb.dp, ee_b, acc);
    };
    // FOUR pairs per trip while eight closed-form dates remain: P = 4g + {0, 1, 2, 3} makes the cursor's phase a compile-time
    // constant in each of the four copies -- no four-way switch, and the carried words are plain values instead of loop-carried
    // copies (the one-pair loop below spends 8 v_mov_b32 + 3 v_mov_b64 of its 216 instructions per trip on them).
    // (the Philox cursors only: a sequential or external stream has no phase switch, and four copies cost it 13 to 90 VGPRs)
    int j = 0;
    if constexpr (Gen::cursor_phases > 1) {
#pragma unroll 1
        for (; j + 8 <= o.n_bs; j += 8) {
            const uint32_t g4 = (uint32_t)(j >> 3) << 2;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                double z0, z1;
                gen.pair(w, c0, 3u /*MC_DOMAIN_CVA*/, g4 | k, carry, z0, z1);
                closed_pair(j + 2 * (int)k, z0, z1);
            }
        }
    }
#pragma unroll 1
    for (; j < n_dates; j += 2) {
        double z0, z1;
        gen.pair(w, c0, 3u /*MC_DOMAIN_CVA*/, (uint32_t)(j >> 1), carry, z0, z1);
        if (j + 1 < o.n_bs) {  // wave-uniform: both dates of this pair have a closed-form exposure
            closed_pair(j, z0, z1);
        } else {
            cva_single_date<double, ANTI>(o, j, n_dates, z0, W, acc);
            cva_single_date<double, ANTI>(o, j + 1, n_dates, z1, W, acc);
        }
    }
    gen.pairs_done((uint32_t)((n_dates + 1) >> 1));
    return acc * (ANTI ? o.lgd * 0.5 : o.lgd);
}

// one lane per path, grid-stride over the segment's paths: workgroup `block` of `n_blocks` (the whole grid for cva_kernel, the
// main part of it for cva_split_kernel)
// `lds_raw`: the launch's dynamic LDS.  fp32 with o.pairs_in_lds: the pair rows are staged there once per workgroup (all threads; a barrier)
template <class Real, bool ANTI, class Gen>
__device__ __forceinline__ void cva_paths_role(const CvaArgs<Real> &o, const Work &w, Real *__restrict__ out, uint32_t block, uint32_t n_blocks,
                                               unsigned char *lds_raw, double &acc_s, double &acc_q)
{
    const uint32_t stride = n_blocks * GROUP;
    const uint32_t gtid = block * GROUP + threadIdx.x;
    [[maybe_unused]] const float *lds_pairs = nullptr;
    if constexpr (sizeof(Real) == 4 && !ANTI) {   // (the antithetic form holds a row across two exposures: measured 0.5 % slower from LDS)
        if (o.pairs_in_lds) {   // uniform over the launch
            float *dst = reinterpret_cast<float *>(lds_raw);
            for (int k = threadIdx.x; k < 12 * (o.n_bs / 2); k += GROUP)
                dst[k] = o.pairs[k];
            __syncthreads();
            lds_pairs = dst;
        }
    }
    Gen gen(w);
    for (uint32_t i = gtid; i < w.n_units; i += stride) {
        Real p;
        if constexpr (sizeof(Real) == 4 && !ANTI)
            p = cva_path<ANTI>(gen, o, w, w.unit_lo + i, lds_pairs);
        else
            p = cva_path<ANTI>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
}

template <class Real, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void cva_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const CvaArgs<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double acc_s = 0.0, acc_q = 0.0;
    cva_paths_role<Real, ANTI, Gen>(o, w, out, blockIdx.x, gridDim.x, lds_raw, acc_s, acc_q);
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// Arithmetic-average (Asian) call on m equally spaced dates, with the geometric average as control variate.  Not in the
// reference.  The walk is cva_path's -- W_j = z_1 + ... + z_j the lane's only state, ln S_j = fma(W_j, bx, xk_j) with
// xk_j = ln S0 + j a from a per-date table (fp64 on the host, rounded once; wave-uniform j: scalar loads, so xk_j is the
// scalar operand of the fma and costs the vector pipe nothing) -- and a date's work is a strict subset of the CVA's: ONE
// exponential, no Hastings tails.  Per path:
//   A = (1/m) sum_j S_j,   value = (A - K)^+
//   CV:   G = E(g0 + g1 sum_j W_j)  (= exp((1/m) sum_j ln S_j): one add per date, one exponential per path),  value -= (G - K)^+
//   ANTI: the same at -z (W -> -W: a second exponential per date, -sum W for the mirrored G), value = mean of the two
// Stream: domain 4, date j (0-based here) = entry j % NPB of block j / NPB: the CVA layout.
// =========================================================================================
template <class Real>
struct AsianArgs {
    const Real *xk;   // n_dates values: (ln S0 + (j + 1) a) in exponent units (natural log in f64, log2 in f32)
    int n_dates;
    Real bx;          // v sqrt(dt) in exponent units
    Real strike;
    Real inv_m;       // 1 / n_dates
    Real g0, g1;      // ln G = g0 + g1 sum_j W_j in exponent units: g0 = ln S0 + a (m + 1) / 2, g1 = bx / m
};

template <class Real>
__device__ __forceinline__ Real asian_value(Real sum, Real sw, const AsianArgs<Real> &o, bool cv)
{
    const Real a = fma_r(sum, o.inv_m, -o.strike);
    Real val = a > 0 ? a : 0;
    if (cv) {
        const Real g = exp_model(fma_r(sw, o.g1, o.g0)) - o.strike;
        val -= g > 0 ? g : 0;
    }
    return val;
}

// fp32: a block of four normals = two packed date pairs per trip, as cva_path<float>: Wp = {W + z0, W + z0 + z1}, one
// v_pk_fma_f32 for the pair's ln2 S (its addend the pair's {xk, xk'} straight from two adjacent SGPRs), two v_exp_f32, one packed add
// into the even / odd halves of sum S, and under CV one packed add into sum W.
template <bool ANTI, bool CV, class Gen>
__device__ __forceinline__ float asian_path(Gen &gen, const AsianArgs<float> &o, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<float>();
    static_assert(NPB == 4, "two packed date pairs per block");
    const int n = o.n_dates;
    // bx in a vector register pair for the whole path: a packed fma reads ONE scalar operand, and that is the pair's {xk, xk'}
    // (left to itself hipcc keeps bx scalar and copies every xk pair into vector registers: 3 v_mov per four dates)
    f2 bx = bcast(o.bx);
    asm("" : "+v"(bx));
    float W = 0;
    f2 sum = {0.0f, 0.0f}, sum_m = {0.0f, 0.0f}, sw = {0.0f, 0.0f};   // even / odd dates
    float z[NPB];
    auto pair = [&](int j, float z0, float z1) {
        const f2 Wp = {W + z0, (W + z0) + z1};
        W = Wp.y;
        const f2 xk = {o.xk[j], o.xk[j + 1]};
        sum += pk_exp2(pk_fma(Wp, bx, xk));
        if (ANTI)
            sum_m += pk_exp2(pk_fma(-Wp, bx, xk));
        if (CV)
            sw += Wp;
    };
    int j0 = 0;
    for (; j0 + NPB <= n; j0 += NPB) {
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 4u /*MC_DOMAIN_ASIAN*/, z);
        pair(j0, z[0], z[1]);
        pair(j0 + 2, z[2], z[3]);
    }
    if (j0 < n) {   // wave-uniform: one to three dates left
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 4u /*MC_DOMAIN_ASIAN*/, z);
        if (j0 + 2 <= n) {
            pair(j0, z[0], z[1]);
            j0 += 2;
        }
        if (j0 < n) {
            W += j0 & 2 ? z[2] : z[0];
            const float xk = o.xk[j0];
            sum.x += __builtin_amdgcn_exp2f(__builtin_fmaf(W, o.bx, xk));
            if (ANTI)
                sum_m.x += __builtin_amdgcn_exp2f(__builtin_fmaf(-W, o.bx, xk));
            if (CV)
                sw.x += W;
        }
    }
    const float sw1 = sw.x + sw.y;
    float val = asian_value(sum.x + sum.y, sw1, o, CV);
    if (ANTI)
        val = 0.5f * (val + asian_value(sum_m.x + sum_m.y, -sw1, o, CV));
    return val;
}

// fp64: dates in Box-Muller pairs through the generator's pair cursor, four pairs per trip for the bulk (the cursor's phase a
// compile-time constant in each copy), one pair per trip for the rest: cva_path<double>'s loop.  bx (and -bx for the mirrored
// path) sit in vector registers for the whole path, so ln S = fma(W, bx, xk_j) reads xk_j from its SGPR pair.
template <bool ANTI, bool CV, class Gen>
__device__ __forceinline__ double asian_path(Gen &gen, const AsianArgs<double> &o, const Work &w, uint32_t c0)
{
    const int n = o.n_dates;
    double W = 0, s_a = 0, s_b = 0, m_a = 0, m_b = 0, sw = 0;   // sum S over even / odd dates, the same for the mirrored path, sum W
    const double bx_v = to_vgpr(o.bx);
    [[maybe_unused]] const double nbx_v = to_vgpr(-o.bx);
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    auto date = [&](int j, double z, double &s, double &m) {
        W += z;
        const double xk = o.xk[j];
        s += exp_f64(fma_scalar_addend(W, bx_v, xk));
        if (ANTI)
            m += exp_f64(fma_scalar_addend(W, nbx_v, xk));
        if (CV)
            sw += W;
    };
    int j = 0;
    if constexpr (Gen::cursor_phases > 1) {
#pragma unroll 1
        for (; j + 8 <= n; j += 8) {
            const uint32_t g4 = (uint32_t)(j >> 3) << 2;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                double z0, z1;
                gen.pair(w, c0, 4u /*MC_DOMAIN_ASIAN*/, g4 | k, carry, z0, z1);
                date(j + 2 * (int)k, z0, s_a, m_a);
                date(j + 2 * (int)k + 1, z1, s_b, m_b);
            }
        }
    }
#pragma unroll 1
    for (; j < n; j += 2) {
        double z0, z1;
        gen.pair(w, c0, 4u /*MC_DOMAIN_ASIAN*/, (uint32_t)(j >> 1), carry, z0, z1);
        date(j, z0, s_a, m_a);
        if (j + 1 < n)   // wave-uniform
            date(j + 1, z1, s_b, m_b);
    }
    gen.pairs_done((uint32_t)((n + 1) >> 1));
    double val = asian_value(s_a + s_b, sw, o, CV);
    if (ANTI)
        val = 0.5 * (val + asian_value(m_a + m_b, -sw, o, CV));
    return val;
}

// one lane per path, grid-stride over the segment's paths
template <class Real, bool ANTI, bool CV, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void asian_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const AsianArgs<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = asian_path<ANTI, CV>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// Single-barrier call on m equally spaced dates, monitored on the dates (CONT = false) or continuously through the
// Brownian-bridge survival probability between them (CONT = true).  Not in the reference.  The walk is asian_path's, but in
// LOG space: the lane's state is W_j and the running minimum of the distance to the barrier
//   d_j = sgn (ln B - ln S_j) = fma(W_j, dbx, dk_j),   dbx = -sgn bx,   dk_j = sgn (ln B - ln S0 - j a)
// (natural-log units; dk_j from the per-date table, folded in fp64 and rounded once -- small exactly where the path is near
// the barrier, so d_j is well conditioned there; wave-uniform j: scalar loads, the fma's one scalar operand).  The direction
// lives in the table and in the sign of dbx: up and down barriers run the same code.  Per path:
//   discrete:    P = [min_j d_j > 0]                                             no transcendental in the date loop
//   continuous:  P = [min_j d_j > 0] prod_j (1 - E(cexp d_{j-1} d_j)),  cexp = -2 / bx^2 (times log2 e in f32), d_0 from the host:
//                one exponential per date.  On a crossed interval d_{j-1} d_j < 0 and the exponential may overflow; P is taken by
//                a SELECT on min d_j > 0, never by a multiply, so inf and NaN stay out and a crossed path has P = 0 exactly
//   value = (c0 + c1 P) (S_T - K)^+,  S_T = E(xT + bxe W_m): (c0, c1) = (0, 1) knock-out, (1, -1) knock-in, wave-uniform
//   ANTI: the same at -z (d^-_j = fma(W_j, -dbx, dk_j)), value = mean of the two
// Stream: domain 5, date j (0-based here) = entry j % NPB of block j / NPB: the Asian layout.
// =========================================================================================
template <class Real>
struct BarrierArgs {
    const Real *dk;   // n_dates values: sgn (ln B - ln S0 - (j + 1) a), natural-log units
    int n_dates;
    Real dbx;         // -sgn v sqrt(dt), natural-log units
    Real d0;          // sgn (ln B - ln S0) > 0: the distance at t_0, where the first bridge starts
    Real cexp;        // -2 / bx^2 in the exponential's units (f32: times log2 e, so the product goes straight into v_exp_f32)
    Real xT, bxe;     // ln S_T = xT + bxe W_m in exponent units (natural log in f64, log2 in f32)
    Real strike;
    Real c0, c1;      // value = (c0 + c1 P) payoff
};

// the survival factor of the running distances is folded by barrier_value: P, then the payoff at maturity
template <bool CONT, class Real>
__device__ __forceinline__ Real barrier_value(Real mn, Real prod, Real W, const BarrierArgs<Real> &o)
{
    const Real live = CONT ? prod : (Real)1;
    const Real P = mn > 0 ? live : (Real)0;   // the select: a NaN or inf product of a crossed path never reaches the value
    const Real pay = exp_model(fma_r(W, o.bxe, o.xT)) - o.strike;
    return fma_r(o.c1, P, o.c0) * (pay > 0 ? pay : 0);
}

// fp32: a block of four normals = two packed date pairs per trip, as asian_path<float>: Wp = {W + z0, W + z0 + z1}, one
// v_pk_fma_f32 for the pair's distances (its addend the pair's {dk, dk'} from two adjacent SGPRs), one v_min3_f32 for the
// running minimum (gfx950 has no packed fp32 min).  CONT adds per pair: one packed multiply by cexp, one packed multiply
// by the previous distances, two v_exp_f32 and one packed fma prod (1 - e) into the even / odd halves of the product.
template <bool ANTI, bool CONT, class Gen>
__device__ __forceinline__ float barrier_path(Gen &gen, const BarrierArgs<float> &o, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<float>();
    static_assert(NPB == 4, "two packed date pairs per block");
    const int n = o.n_dates;
    // dbx in a vector register pair for the whole path: the packed fma's ONE scalar operand is the pair's {dk, dk'}
    f2 dbx = bcast(o.dbx);
    asm("" : "+v"(dbx));
    const f2 one = bcast(1.0f);
    [[maybe_unused]] const f2 cexp = bcast(o.cexp);
    float W = 0, mn = __builtin_inff(), mn_m = __builtin_inff();
    float tp = o.cexp * o.d0, tp_m = tp;              // cexp d_{j-1} of the last date seen
    f2 prod = one, prod_m = one;                      // even / odd dates
    float z[NPB];
    auto side = [&](f2 d, float &mn_, float &tp_, f2 &prod_) {
        mn_ = __builtin_fminf(__builtin_fminf(mn_, d.x), d.y);
        if (CONT) {
            const f2 t = d * cexp;
            const f2 u = (f2){tp_, t.x} * d;
            prod_ = pk_fma(-prod_, pk_exp2(u), prod_);   // prod (1 - e)
            tp_ = t.y;
        }
    };
    auto pair = [&](int j, float z0, float z1) {
        const f2 Wp = {W + z0, (W + z0) + z1};
        W = Wp.y;
        const f2 dk = {o.dk[j], o.dk[j + 1]};
        side(pk_fma(Wp, dbx, dk), mn, tp, prod);
        if (ANTI)
            side(pk_fma(-Wp, dbx, dk), mn_m, tp_m, prod_m);
    };
    auto single = [&](float d, float &mn_, float &tp_, f2 &prod_) {
        mn_ = __builtin_fminf(mn_, d);
        if (CONT) {
            prod_.x = __builtin_fmaf(-prod_.x, __builtin_amdgcn_exp2f(tp_ * d), prod_.x);
            tp_ = o.cexp * d;
        }
    };
    int j0 = 0;
    for (; j0 + NPB <= n; j0 += NPB) {
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 5u /*MC_DOMAIN_BARRIER*/, z);
        pair(j0, z[0], z[1]);
        pair(j0 + 2, z[2], z[3]);
    }
    if (j0 < n) {   // wave-uniform: one to three dates left
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 5u /*MC_DOMAIN_BARRIER*/, z);
        if (j0 + 2 <= n) {
            pair(j0, z[0], z[1]);
            j0 += 2;
        }
        if (j0 < n) {
            W += j0 & 2 ? z[2] : z[0];
            const float dk = o.dk[j0];
            single(__builtin_fmaf(W, o.dbx, dk), mn, tp, prod);
            if (ANTI)
                single(__builtin_fmaf(-W, o.dbx, dk), mn_m, tp_m, prod_m);
        }
    }
    float val = barrier_value<CONT>(mn, prod.x * prod.y, W, o);
    if (ANTI)
        val = 0.5f * (val + barrier_value<CONT>(mn_m, prod_m.x * prod_m.y, -W, o));
    return val;
}

// min(a, b) of two doubles that are never signalling NaNs, as ONE v_min_f64 (hipcc puts a canonicalising v_max_f64 in front of the
// running minimum's __builtin_fmin on every date)
__device__ __forceinline__ double min_f64(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// fp64: asian_path<double>'s loop (Box-Muller pairs through the generator's pair cursor, four pairs per trip, then one): per
// date one add, one v_fma_f64 with dk_j from its SGPR pair and one v_min_f64.  CONT: the exponent is clamped from below
// (exp_f64's argument range; a live path's exponent is negative and e^-800 is 0 anyway), what a crossed interval gives is dropped
// by the select.
template <bool ANTI, bool CONT, class Gen>
__device__ __forceinline__ double barrier_path(Gen &gen, const BarrierArgs<double> &o, const Work &w, uint32_t c0)
{
    const int n = o.n_dates;
    double W = 0, mn = __builtin_inf(), mn_m = __builtin_inf(), prod = 1.0, prod_m = 1.0;
    double tp = o.cexp * o.d0, tp_m = tp;
    const double dbx_v = to_vgpr(o.dbx);
    [[maybe_unused]] const double ndbx_v = to_vgpr(-o.dbx);
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    auto side = [&](double d, double &mn_, double &tp_, double &prod_) {
        mn_ = min_f64(mn_, d);
        if (CONT) {
            const double u = __builtin_fmax(tp_ * d, -800.0);
            prod_ = __builtin_fma(-prod_, exp_f64(u), prod_);
            tp_ = o.cexp * d;
        }
    };
    auto date = [&](int j, double z) {
        W += z;
        const double dk = o.dk[j];
        side(fma_scalar_addend(W, dbx_v, dk), mn, tp, prod);
        if (ANTI)
            side(fma_scalar_addend(W, ndbx_v, dk), mn_m, tp_m, prod_m);
    };
    int j = 0;
    if constexpr (Gen::cursor_phases > 1) {
#pragma unroll 1
        for (; j + 8 <= n; j += 8) {
            uint32_t blk = (uint32_t)(j >> 3);
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                // discrete form: a pair's generator call starts after the running minimum of the pair before it (its block index
                // passes through the same empty statement).  Left free, hipcc overlaps the four calls around the few
                // instructions of the dates and needs 129 vector registers: three waves per SIMD instead of four.  (A scheduling
                // barrier does the same but counts as a memory write, which turns the table's scalar loads into vector loads.)
                if (!CONT && k)
                    asm("" : "+v"(mn), "+s"(blk));
                double z0, z1;
                gen.pair(w, c0, 5u /*MC_DOMAIN_BARRIER*/, (blk << 2) | k, carry, z0, z1);
                date(j + 2 * (int)k, z0);
                date(j + 2 * (int)k + 1, z1);
            }
        }
    }
#pragma unroll 1
    for (; j < n; j += 2) {
        double z0, z1;
        gen.pair(w, c0, 5u /*MC_DOMAIN_BARRIER*/, (uint32_t)(j >> 1), carry, z0, z1);
        date(j, z0);
        if (j + 1 < n)   // wave-uniform
            date(j + 1, z1);
    }
    gen.pairs_done((uint32_t)((n + 1) >> 1));
    double val = barrier_value<CONT>(mn, prod, W, o);
    if (ANTI)
        val = 0.5 * (val + barrier_value<CONT>(mn_m, prod_m, -W, o));
    return val;
}

// one lane per path, grid-stride over the segment's paths.  Four waves per SIMD at least, asian_kernel's occupancy in fp64: left to
// itself hipcc spends 129 vector registers on the fp64 discrete forms (one more than four waves allow) on a loop that needs fewer.
template <class Real, bool ANTI, bool CONT, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void barrier_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const BarrierArgs<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = barrier_path<ANTI, CONT>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// Worst-of / best-of ("rainbow") options on NA correlated assets walked over m equally spaced dates, with an optional barrier on
// the same extremum, monitored on the dates (the model is stated in mc_mi355x.h).  Not in the reference.  basket_kernel's
// host-folded Cholesky step joined to barrier_path's walk in LOG space: the lane's state is W_0 ... W_{NA-1} (one running sum of
// normals per factor) and the running minimum of the distance to the barrier, nothing else.  Per date j
//   cs_i = sum_{k<=i} me_ik W_k                 me = e diag(v sqrt dt) L, kernel arguments, NA (NA + 1) / 2 fmas
//   Y    = max_i (tab_ji + cs_i)                tab_ji = e (ln(w_i s_i) + j a_i) from the per-date table (constant address space:
//                                               scalar loads); e = -1 looks at the minimum, +1 at the maximum: both run the same code
//   d_j  = fma(g, Y, bl)                        g = -b e, bl = b ln B; running minimum by one v_min
// and no transcendental.  After the last date P = [min_j d_j > 0] by a select, X = E(esc Y_m) (esc = e times the exponent's unit),
//   value = (c0 + c1 P) max(q (X - K), 0)       (c0, c1, q wave-uniform: no kernel per type; no barrier is g = bl = c1 = 0)
//   ANTI: the same at -z (tab_ji - cs_i: the correlated sums are formed once), value = mean of the two
// Stream: domain 14, the normal of date j (0-based here) and factor k is FLAT entry j NA + k of the Asian layout: entry % NPB of
// block / NPB, in fp64 the pair cursor's pair entry >> 1.  The phase of a date's first entry repeats every NPB / gcd(NA, NPB) dates
// (fp64: pairs, every 2 / gcd(NA, 2) dates): that many dates are unrolled per trip, so every entry of a trip sits at a
// compile-time place of its block or pair, and the dates left over start a block or pair of their own.
// =========================================================================================
template <class Real, int NA>
struct RainbowArgs {
    const Real *tab;             // n_dates rows of NA values: e (ln(w_i s_i) + (j + 1) a_i), natural-log units
    int n_dates;
    Real me[NA * (NA + 1) / 2];  // e v_i sqrt(dt) L_ik, lower triangle by rows, natural-log units
    Real g, bl;                  // d_j = g Y_j + bl
    Real esc;                    // e in exponent units (natural log in f64, log2 in f32)
    Real q, strike;
    Real c0, c1;                 // value = (c0 + c1 P) payoff
};
template <class Real> using RainbowRowPtr = const __attribute__((address_space(4))) Real *;

__device__ __forceinline__ double max_f64(double a, double b);   // ONE v_max_f64, defined with the lookback options below
__device__ __forceinline__ float rainbow_max(float a, float b) { return __builtin_fmaxf(a, b); }   // pairs of them fuse into v_max3_f32
__device__ __forceinline__ double rainbow_max(double a, double b) { return max_f64(a, b); }
__device__ __forceinline__ float rainbow_min(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double rainbow_min(double a, double b) { return min_f64(a, b); }

constexpr int rainbow_gcd(int a, int b) { return b ? rainbow_gcd(b, a % b) : a; }

// Where the coefficients me live was decided per precision and size on the `make asm` listing and then on the clock (DESIGN
// 4.14, profiles/rainbow_ab.log): kernel arguments, the scalar operand of the fmas, at every size.  fp32: no spill reload in any
// bulk loop.  fp64: from NA = 4 M's SGPR pairs spill beside the generator's (4 ... 124 SGPRs, their v_readlane reloads in the date
// loop) and from NA = 5 hipcc overlaps the trip's generator calls (three waves per SIMD).  A copy of M staged in LDS
// (basket_consts_in_lds's remedy) removed every spill and 4.8's empty-asm tie between the generator calls gave four waves at
// NA = 3 ... 6 -- and both were SLOWER: LDS 4 to 9 % at NA = 3 ... 7 (level at NA = 8: 1.4 % faster, inside the spread, and only in
// a form that spilled to scratch), the tie 2 to 4 % (12 % at NA = 8), both together 3 to 10 %.  The walk is bound by the vector pipe: overlapped generator calls are worth more to it than a fourth wave,
// and a v_readlane costs less than a ds_read and its wait.  Asking for four waves (amdgpu_waves_per_eu) at NA = 7, 8 spills vector
// registers to scratch.  None of the three is in the code.

// one date: the extremum of the NA log levels from the factors' running sums, and the running minimum of the distance
template <bool ANTI, class Real, int NA>
__device__ __forceinline__ void rainbow_date(const RainbowArgs<Real, NA> &o, RainbowRowPtr<Real> row, const Real (&W)[NA], Real &Y, Real &Y_m,
                                             Real &mn, Real &mn_m)
{
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        Real cs = o.me[i * (i + 1) / 2] * W[0];
#pragma unroll
        for (int k = 1; k <= i; ++k)
            cs = fma_r(o.me[i * (i + 1) / 2 + k], W[k], cs);
        const Real t = row[i];
        Y = i ? rainbow_max(Y, t + cs) : t + cs;
        if (ANTI)
            Y_m = i ? rainbow_max(Y_m, t - cs) : t - cs;
    }
    mn = rainbow_min(mn, fma_r(o.g, Y, o.bl));
    if (ANTI)
        mn_m = rainbow_min(mn_m, fma_r(o.g, Y_m, o.bl));
}

template <class Real, int NA>
__device__ __forceinline__ Real rainbow_value(Real mn, Real Y, const RainbowArgs<Real, NA> &o)
{
    const Real P = mn > 0 ? (Real)1 : (Real)0;
    const Real pay = o.q * (exp_model(o.esc * Y) - o.strike);
    return fma_r(o.c1, P, o.c0) * (pay > 0 ? pay : 0);
}

// fp32: blocks of four normals; NPB / gcd(NA, NPB) = 4, 2 or 1 dates per trip for NA odd, = 2 mod 4, = 0 mod 4
template <bool ANTI, int NA, class Gen>
__device__ __forceinline__ float rainbow_path(Gen &gen, const RainbowArgs<float, NA> &o, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<float>();
    constexpr int U = NPB / rainbow_gcd(NA, NPB), BPT = U * NA / NPB;   // dates and blocks per trip
    const int n = o.n_dates;
    const RainbowRowPtr<float> tab = (RainbowRowPtr<float>)o.tab;
    float W[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k)
        W[k] = 0;
    float Y = 0, Y_m = 0, mn = __builtin_inff(), mn_m = __builtin_inff();
    float z[NPB];
    // date d of the trip that starts at date j and block blk: entries d NA ... d NA + NA - 1 of the trip, places known at compile time
    auto date = [&](int d, int j, uint32_t blk) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int e = d * NA + k;
            if (e % NPB == 0)
                gen.normals(w, c0, blk + (uint32_t)(e / NPB), 14u /*MC_DOMAIN_RAINBOW*/, z);
            W[k] += z[e % NPB];
        }
        rainbow_date<ANTI>(o, tab + (j + d) * NA, W, Y, Y_m, mn, mn_m);
    };
    int j = 0;
    uint32_t blk = 0;
#pragma unroll 1
    for (; j + U <= n; j += U, blk += BPT) {
#pragma unroll
        for (int d = 0; d < U; ++d)
            date(d, j, blk);
    }
#pragma unroll
    for (int d = 0; d < U - 1; ++d)   // wave-uniform: up to U - 1 dates left, the first at the start of a block
        if (j + d < n)
            date(d, j, blk);
    float val = rainbow_value(mn, Y, o);
    if (ANTI)
        val = 0.5f * (val + rainbow_value(mn_m, Y_m, o));
    return val;
}

// fp64: Box-Muller pairs through the generator's pair cursor, drawn strictly in order; two dates per trip for odd NA (its second
// date starts on the second normal of a pair), one for even NA.  The cursor's four-phase state is resolved by a scalar branch per
// pair (asian_path<double>'s remainder loop).  A bulk loop of 8 / gcd(NA, 8) dates with compile-time phases was built and dropped
// on the listing: it cost vector registers at NA = 1, 2 (92 -> 99 and 126, four waves for five), gained none at NA = 3, 5, 7 and
// doubled the code; with the tie and the LDS copy it took 121 registers for 100 at NA = 4 and three waves at NA = 6.
template <bool ANTI, int NA, class Gen>
__device__ __forceinline__ double rainbow_path(Gen &gen, const RainbowArgs<double, NA> &o, const Work &w, uint32_t c0)
{
    constexpr int U = 2 / rainbow_gcd(NA, 2), PPT = U * NA / 2;   // dates and pairs per trip
    const int n = o.n_dates;
    const RainbowRowPtr<double> tab = (RainbowRowPtr<double>)o.tab;
    double W[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k)
        W[k] = 0;
    double Y = 0, Y_m = 0, mn = __builtin_inf(), mn_m = __builtin_inf();
    double zp[2];
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    auto date = [&](int d, int j, uint32_t pr) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int e = d * NA + k;
            if (e % 2 == 0)
                gen.pair(w, c0, 14u /*MC_DOMAIN_RAINBOW*/, pr + (uint32_t)(e / 2), carry, zp[0], zp[1]);
            W[k] += zp[e % 2];
        }
        rainbow_date<ANTI>(o, tab + (j + d) * NA, W, Y, Y_m, mn, mn_m);
    };
    int j = 0;
    uint32_t pr = 0;
#pragma unroll 1
    for (; j + U <= n; j += U, pr += PPT) {
#pragma unroll
        for (int d = 0; d < U; ++d)
            date(d, j, pr);
    }
    if (U > 1 && j < n)   // wave-uniform: odd NA and an odd number of dates; the last pair's second normal is not used
        date(0, j, pr);
    gen.pairs_done((uint32_t)((n * NA + 1) >> 1));
    double val = rainbow_value(mn, Y, o);
    if (ANTI)
        val = 0.5 * (val + rainbow_value(mn_m, Y_m, o));
    return val;
}

// one lane per path, grid-stride over the segment's paths: barrier_kernel's frame
template <class Real, int NA, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void rainbow_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const RainbowArgs<Real, NA> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = rainbow_path<ANTI, NA>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// Worst-of autocallable notes on NA correlated assets: memory coupons, early redemption on observation dates and a knock-in put at
// maturity (the model is stated in mc_mi355x.h).  Not in the reference.  rainbow_path's walk with the extremum fixed to the
// minimum, in the same trips of compile-time phases, but the path PAYS ON THE WAY and may end before the last date.  Per date j
//   y = min_i (tab_ji + cs_i),  mn = min(mn, y)         tab_ji = ln(w_i s_i) + j a_i, cs_i as in the rainbow's step (me = +M)
// and, where date j is the next observation (a wave-uniform compare of two integers, one scalar branch), for observation k < n_obs
//   called = [y >= LA_k],  paid = [y >= LP_k]            LA_k = ln A_k, LP_k = ln min(A_k, C_k): +-inf allowed, compared directly
//   cash = paid ? fma(cm, miss, c) : 0                   cm = c memory;  miss = paid ? 0 : miss + 1
//   V = fma(alive D_k, cash + called, V)                 D_k = exp(-r t_kE), folded on the host;  alive = called ? 0 : alive
// (LA_k, LP_k, D_k: three values per observation behind the per-date rows of the same table, scalar loads).  After the last date
//   KI = [(ki_dates ? mn : y) <= lb]                     lb = ln B, +inf without a knock-in condition
//   V = fma(alive D, fma(-(KI ? g : 0), max(K - E(esc y), 0), cash + 1), V)
// so the date loop holds no transcendental, every decision is a compare of the log level against a table value, and alive, miss
// and V move by selects and fmas.  ANTI: the same at -z, value = mean of the two.
// Early exit (MC_AUTOCALL_EARLY_EXIT, compiled OUT): after an observation a wave none of whose lanes is alive in either direction
// can leave the date loop; what it skips would be multiplied by alive = 0, so no value changes.  The stream is counter-based
// (GenPhilox: every block and pair is addressed by its index, the pair cursor's carry is refilled at pair 0 of the next path and
// pairs_done does nothing), so drawing fewer entries than n NA needs no bookkeeping; the generators that keep a sequence are refused
// by the host.  Built and timed against the kernel without it (tools/autocall_speed.py, profiles/autocall_ab.log): a
// wave leaves only when all of its 64 paths are called, which a traded note's schedule never brings about (a third of its paths
// reach maturity), so the exit bought nothing on it and cost its ballot per observation; it stays a switch of the build.
// Stream: domain 15, the rainbow's flat (date, factor) layout.
// =========================================================================================
#ifndef MC_AUTOCALL_EARLY_EXIT
#define MC_AUTOCALL_EARLY_EXIT 0   // decided on the clock: DESIGN 4.15, profiles/autocall_ab.log
#endif

template <class Real, int NA>
struct AutocallArgs {
    const Real *tab;             // n_dates rows of NA values ln(w_i s_i) + (j + 1) a_i, then n_obs rows (LA_k, LP_k, D_k)
    int n_dates, n_obs, every;   // every = n_dates / n_obs walk dates per observation
    int ki_dates;                // the knock-in looks at the minimum over all dates (1) or at the level at maturity (0)
    Real me[NA * (NA + 1) / 2];  // v_i sqrt(dt) L_ik, lower triangle by rows, natural-log units
    Real lb;                     // ln B; +inf: the put is always live
    Real esc;                    // the exponent's unit (natural log in f64, log2 in f32)
    Real strike, g;
    Real c, cm;                  // the coupon, and the coupon times the memory switch
};

// what one path direction carries between the dates
template <class Real>
struct AutocallSide {
    Real y, mn, alive, miss, V;
};

// one date: the minimum of the NA log levels from the factors' running sums, and its running minimum (rainbow_date's step)
template <bool ANTI, class Real, int NA>
__device__ __forceinline__ void autocall_date(const AutocallArgs<Real, NA> &o, RainbowRowPtr<Real> row, const Real (&W)[NA], AutocallSide<Real> &p,
                                              AutocallSide<Real> &q)
{
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        Real cs = o.me[i * (i + 1) / 2] * W[0];
#pragma unroll
        for (int k = 1; k <= i; ++k)
            cs = fma_r(o.me[i * (i + 1) / 2 + k], W[k], cs);
        const Real t = row[i];
        p.y = i ? rainbow_min(p.y, t + cs) : t + cs;
        if (ANTI)
            q.y = i ? rainbow_min(q.y, t - cs) : t - cs;
    }
    p.mn = rainbow_min(p.mn, p.y);
    if (ANTI)
        q.mn = rainbow_min(q.mn, q.y);
}

template <class Real, int NA>
__device__ __forceinline__ Real autocall_cash(const AutocallArgs<Real, NA> &o, Real LP, AutocallSide<Real> &p)
{
    const bool paid = p.y >= LP;
    const Real cash = paid ? fma_r(o.cm, p.miss, o.c) : (Real)0;
    p.miss = paid ? (Real)0 : p.miss + (Real)1;
    return cash;
}

// an observation before the last: the coupon, and the redemption of a path that is called
template <class Real, int NA>
__device__ __forceinline__ void autocall_observe(const AutocallArgs<Real, NA> &o, RainbowRowPtr<Real> obs, AutocallSide<Real> &p)
{
    const Real LA = obs[0], LP = obs[1], D = obs[2];
    const bool called = p.y >= LA;
    const Real cash = autocall_cash(o, LP, p);
    p.V = fma_r(p.alive * D, cash + (called ? (Real)1 : (Real)0), p.V);
    p.alive = called ? (Real)0 : p.alive;
}

// the last observation: the coupon, the notional and the knock-in put
template <class Real, int NA>
__device__ __forceinline__ Real autocall_maturity(const AutocallArgs<Real, NA> &o, RainbowRowPtr<Real> obs, AutocallSide<Real> &p)
{
    const Real LP = obs[1], D = obs[2];
    const Real cash = autocall_cash(o, LP, p);
    const Real gk = (o.ki_dates ? p.mn : p.y) <= o.lb ? o.g : (Real)0;
    const Real put = o.strike - exp_model(o.esc * p.y);
    return fma_r(p.alive * D, fma_r(-gk, put > 0 ? put : (Real)0, cash + (Real)1), p.V);
}

template <bool ANTI, class Real>
__device__ __forceinline__ bool autocall_wave_dead(const AutocallSide<Real> &p, const AutocallSide<Real> &q)
{
    return __builtin_amdgcn_ballot_w64(p.alive != 0 || (ANTI && q.alive != 0)) == 0;
}

template <class Real>
__device__ __forceinline__ AutocallSide<Real> autocall_start()
{
    return AutocallSide<Real>{(Real)0, (Real)__builtin_inf(), (Real)1, (Real)0, (Real)0};
}

// fp32: blocks of four normals, rainbow_path's trips
template <bool ANTI, int NA, class Gen>
__device__ __forceinline__ float autocall_path(Gen &gen, const AutocallArgs<float, NA> &o, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<float>();
    constexpr int U = NPB / rainbow_gcd(NA, NPB), BPT = U * NA / NPB;   // dates and blocks per trip
    const int n = o.n_dates;
    const RainbowRowPtr<float> tab = (RainbowRowPtr<float>)o.tab, obs = tab + n * NA;
    float W[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k)
        W[k] = 0;
    AutocallSide<float> p = autocall_start<float>(), q = autocall_start<float>();
    float z[NPB];
    int next = o.every, k_obs = 0;   // the date (1-based) of the next observation, and its row
    bool dead = false;               // wave-uniform
    auto date = [&](int d, int j, uint32_t blk) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int e = d * NA + k;
            if (e % NPB == 0)
                gen.normals(w, c0, blk + (uint32_t)(e / NPB), 15u /*MC_DOMAIN_AUTOCALL*/, z);
            W[k] += z[e % NPB];
        }
        autocall_date<ANTI>(o, tab + (j + d) * NA, W, p, q);
        if (j + d + 1 == next && next != n) {   // wave-uniform: the last observation is taken after the loop
            autocall_observe(o, obs + 3 * k_obs, p);
            if (ANTI)
                autocall_observe(o, obs + 3 * k_obs, q);
            next += o.every, ++k_obs;
            if (MC_AUTOCALL_EARLY_EXIT)
                dead = autocall_wave_dead<ANTI>(p, q);
        }
    };
    int j = 0;
    uint32_t blk = 0;
#pragma unroll 1
    for (; j + U <= n && !dead; j += U, blk += BPT) {
#pragma unroll
        for (int d = 0; d < U; ++d)
            date(d, j, blk);
    }
    if (!dead) {
#pragma unroll
        for (int d = 0; d < U - 1; ++d)   // wave-uniform: up to U - 1 dates left, the first at the start of a block
            if (j + d < n)
                date(d, j, blk);
    }
    float val = autocall_maturity(o, obs + 3 * (o.n_obs - 1), p);
    if (ANTI)
        val = 0.5f * (val + autocall_maturity(o, obs + 3 * (o.n_obs - 1), q));
    return val;
}

// fp64: the generator's pair cursor, rainbow_path's trips.  A wave that leaves early has drawn fewer pairs than pairs_done is
// told: the counter-based generators this product is served with ignore the count.
template <bool ANTI, int NA, class Gen>
__device__ __forceinline__ double autocall_path(Gen &gen, const AutocallArgs<double, NA> &o, const Work &w, uint32_t c0)
{
    constexpr int U = 2 / rainbow_gcd(NA, 2), PPT = U * NA / 2;   // dates and pairs per trip
    const int n = o.n_dates;
    const RainbowRowPtr<double> tab = (RainbowRowPtr<double>)o.tab, obs = tab + n * NA;
    double W[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k)
        W[k] = 0;
    AutocallSide<double> p = autocall_start<double>(), q = autocall_start<double>();
    double zp[2];
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    int next = o.every, k_obs = 0;
    bool dead = false;
    auto date = [&](int d, int j, uint32_t pr) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int e = d * NA + k;
            if (e % 2 == 0)
                gen.pair(w, c0, 15u /*MC_DOMAIN_AUTOCALL*/, pr + (uint32_t)(e / 2), carry, zp[0], zp[1]);
            W[k] += zp[e % 2];
        }
        autocall_date<ANTI>(o, tab + (j + d) * NA, W, p, q);
        if (j + d + 1 == next && next != n) {
            autocall_observe(o, obs + 3 * k_obs, p);
            if (ANTI)
                autocall_observe(o, obs + 3 * k_obs, q);
            next += o.every, ++k_obs;
            if (MC_AUTOCALL_EARLY_EXIT)
                dead = autocall_wave_dead<ANTI>(p, q);
        }
    };
    int j = 0;
    uint32_t pr = 0;
#pragma unroll 1
    for (; j + U <= n && !dead; j += U, pr += PPT) {
#pragma unroll
        for (int d = 0; d < U; ++d)
            date(d, j, pr);
    }
    if (U > 1 && j < n && !dead)   // wave-uniform: odd NA and an odd number of dates; the last pair's second normal is not used
        date(0, j, pr);
    gen.pairs_done((uint32_t)((n * NA + 1) >> 1));
    double val = autocall_maturity(o, obs + 3 * (o.n_obs - 1), p);
    if (ANTI)
        val = 0.5 * (val + autocall_maturity(o, obs + 3 * (o.n_obs - 1), q));
    return val;
}

// one lane per path, grid-stride over the segment's paths: rainbow_kernel's frame and reduction
template <class Real, int NA, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void autocall_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const AutocallArgs<Real, NA> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = autocall_path<ANTI, NA>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// Lookback options on m equally spaced dates: the payoff is written on the running maximum or minimum of the spot, taken on
// the dates (CONT = false) or continuously, by sampling the maximum of the Brownian bridge between them (CONT = true).  Not in
// the reference.  barrier_path's walk in LOG space: the lane's state is W_j and the running maximum of the signed excursion
//   y_j = sgn (ln S_j - ln S0) = fma(W_j, sbx, yk_j),   sbx = sgn bx,   yk_j = sgn j a      (y_0 = 0)
// (yk_j from the per-date table, folded in fp64 and rounded once; wave-uniform j: scalar loads, the fma's one scalar operand).
// sgn = +1 looks at the maximum, -1 at the minimum: the direction lives in the table and in the sign of sbx, both run the same code.
//   discrete:    Y = max_{j>=1} y_j                                             one fma and one max per date
//   continuous:  Y = max_j M_j,  2 M_j = y_{j-1} + y_j + sqrt((y_j - y_{j-1})^2 + bx^2 E_j),  E_j = -2 ln u_j: the loop keeps 2 M_j
//                (M_j >= max(y_{j-1}, y_j): the endpoints need no max of their own) and the half goes into the exponent's factor.
//                fp32 walks in natural-log units with bx^2 E_j = e2 log2 u_j (e2 = -2 ln2 bx^2 from the host, box_muller_f32's
//                scale2); fp64 walks in units of bx (sbx = sgn, yk_j = sgn j a / bx), so that sqrt_pos's radicand is
//                (z_j + a/bx)^2 + E_j >= E_j >= 2^-52 whatever the volatility, and the unit goes into the exponent's factor too.
//   ext = S0 E(x0 + es Y) the extremum, S_T = E(x0 + eT y_m) from the walk's own last excursion (so S_T <= the maximum and >= the
//   minimum in floating point as well), value = max(q (ext - R), 0), R = S_T (floating strike) or K (fixed): q and the choice of
//   R are wave-uniform numbers, the four types run the same kernels.
//   ANTI: the same at -z (y^-_j = fma(W_j, -sbx, yk_j)) with the SAME E_j, value = mean of the two
// Stream: normals domain 8, date j (0-based here) = entry j % NPB of block j / NPB: the Asian layout.  Bridge uniforms domain 9,
// raw Philox blocks of the same unit: fp32 date j = word j % 4 of block j / 4, fp64 date j = words 2 (j % 2), 2 (j % 2) + 1 of block j / 2.
// =========================================================================================
template <class Real>
struct LookbackArgs {
    const Real *yk;   // n_dates values: sgn (j + 1) a in the walk's units
    int n_dates;
    Real sbx;         // sgn v sqrt(dt) in the walk's units (fp64 continuous: sgn alone)
    Real e2;          // fp32 continuous: -2 ln2 bx^2; otherwise unused
    Real x0;          // ln S0 in exponent units (natural log in f64, log2 in f32)
    Real es;          // ln ext = x0 + es Y in exponent units: sgn times the walk's unit, halved under CONT (Y is then max 2 M_j)
    Real eT;          // ln S_T = x0 + eT y_m in exponent units: sgn times the walk's unit
    Real strike;
    Real q;           // +1: max(ext - R, 0), -1: max(R - ext, 0)
    int floating;     // R = S_T (1) or the strike (0)
};

template <class Real>
__device__ __forceinline__ Real lookback_value(Real Y, Real y_last, const LookbackArgs<Real> &o)
{
    const Real ext = exp_model(fma_r(Y, o.es, o.x0));
    const Real R = o.floating ? exp_model(fma_r(y_last, o.eT, o.x0)) : o.strike;   // wave-uniform choice
    const Real d = o.q * (ext - R);
    return d > 0 ? d : 0;
}

// fp32: a block of four normals = two packed date pairs per trip, as barrier_path<float>: one v_pk_fma_f32 for the pair's excursions
// (its addend the pair's {yk, yk'} from two adjacent SGPRs) and one v_max3_f32.  CONT draws the four dates' uniforms from one raw
// Philox block and adds per pair: two v_log_f32 and one packed multiply (shared by the mirrored path), then per direction a packed
// subtract, a packed fma (the radicand), two v_sqrt_f32 and two packed adds.
template <bool ANTI, bool CONT, class Gen>
__device__ __forceinline__ float lookback_path(Gen &gen, const LookbackArgs<float> &o, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<float>();
    static_assert(NPB == 4, "two packed date pairs per block");
    const int n = o.n_dates;
    // sbx in a vector register pair for the whole path: the packed fma's ONE scalar operand is the pair's {yk, yk'}
    f2 sbx = bcast(o.sbx);
    asm("" : "+v"(sbx));
    [[maybe_unused]] const f2 e2 = bcast(o.e2);
    float W = 0, Y = -__builtin_inff(), Y_m = -__builtin_inff();
    float yp = 0, yp_m = 0;                           // y_{j-1} of the last date seen
    float z[NPB];
    float u[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    auto side = [&](f2 y, f2 be, float &Y_, float &yp_) {
        if (CONT) {
            const f2 prev = {yp_, y.x};
            const f2 d = y - prev;
            const f2 rad = pk_fma(d, d, be);
            const f2 M2 = (y + prev) + (f2){__builtin_amdgcn_sqrtf(rad.x), __builtin_amdgcn_sqrtf(rad.y)};
            Y_ = __builtin_fmaxf(__builtin_fmaxf(Y_, M2.x), M2.y);
        } else {
            Y_ = __builtin_fmaxf(__builtin_fmaxf(Y_, y.x), y.y);
        }
        yp_ = y.y;
    };
    auto pair = [&](int j, float z0, float z1, float u0, float u1) {
        const f2 Wp = {W + z0, (W + z0) + z1};
        W = Wp.y;
        const f2 yk = {o.yk[j], o.yk[j + 1]};
        f2 be = {0.0f, 0.0f};
        if (CONT)
            be = (f2){__builtin_amdgcn_logf(u0), __builtin_amdgcn_logf(u1)} * e2;
        side(pk_fma(Wp, sbx, yk), be, Y, yp);
        if (ANTI)
            side(pk_fma(-Wp, sbx, yk), be, Y_m, yp_m);
    };
    auto single = [&](float y, float be, float &Y_, float &yp_) {
        if (CONT) {
            const float d = y - yp_;
            Y_ = __builtin_fmaxf(Y_, (y + yp_) + __builtin_amdgcn_sqrtf(__builtin_fmaf(d, d, be)));
        } else {
            Y_ = __builtin_fmaxf(Y_, y);
        }
        yp_ = y;
    };
    int j0 = 0;
    for (; j0 + NPB <= n; j0 += NPB) {
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 8u /*MC_DOMAIN_LOOKBACK*/, z);
        if (CONT)
            gen.uniforms(w, c0, (uint32_t)(j0 / NPB), 9u /*MC_DOMAIN_LOOKBACK_BRIDGE*/, u);
        pair(j0, z[0], z[1], u[0], u[1]);
        pair(j0 + 2, z[2], z[3], u[2], u[3]);
    }
    if (j0 < n) {   // wave-uniform: one to three dates left
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 8u /*MC_DOMAIN_LOOKBACK*/, z);
        if (CONT)
            gen.uniforms(w, c0, (uint32_t)(j0 / NPB), 9u /*MC_DOMAIN_LOOKBACK_BRIDGE*/, u);
        if (j0 + 2 <= n) {
            pair(j0, z[0], z[1], u[0], u[1]);
            j0 += 2;
        }
        if (j0 < n) {
            W += j0 & 2 ? z[2] : z[0];
            const float yk = o.yk[j0];
            const float be = CONT ? o.e2 * __builtin_amdgcn_logf(j0 & 2 ? u[2] : u[0]) : 0.0f;
            single(__builtin_fmaf(W, o.sbx, yk), be, Y, yp);
            if (ANTI)
                single(__builtin_fmaf(-W, o.sbx, yk), be, Y_m, yp_m);
        }
    }
    float val = lookback_value(Y, yp, o);
    if (ANTI)
        val = 0.5f * (val + lookback_value(Y_m, yp_m, o));
    return val;
}

// max(a, b) of two doubles that are never signalling NaNs, as ONE v_max_f64 (min_f64's twin: hipcc puts a canonicalising
// instruction in front of the running maximum's __builtin_fmax on every date)
__device__ __forceinline__ double max_f64(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// c - a * b with c read from its SGPR pair: fma_scalar_addend on the mirrored path, the sign as the instruction's operand modifier
// (a second register pair holding -b is what puts the fp64 antithetic continuous form over 128 vector registers)
__device__ __forceinline__ double fnma_scalar_addend(double a, double b, double c)
{
    double r;
    asm("v_fma_f64 %0, -%1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}

// fp64: barrier_path<double>'s loop (Box-Muller pairs through the generator's pair cursor, four pairs per trip, then one): per
// date one add, one v_fma_f64 with yk_j from its SGPR pair and one v_max_f64.  CONT: a pair of dates draws its two uniforms from
// one raw Philox block, E_j by the table-driven -2 ln u of the normals, and per direction a subtract, the radicand's fma, sqrt_pos
// and two adds.
template <bool ANTI, bool CONT, class Gen>
__device__ __forceinline__ double lookback_path(Gen &gen, const LookbackArgs<double> &o, const Work &w, uint32_t c0)
{
    const int n = o.n_dates;
    double W = 0, Y = -__builtin_inf(), Y_m = -__builtin_inf(), yp = 0, yp_m = 0;
    const double sbx_v = to_vgpr(o.sbx);
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    auto side = [&](double y, double E, double &Y_, double &yp_) {
        if (CONT) {
            const double d = y - yp_;
            Y_ = max_f64(Y_, (y + yp_) + sqrt_pos(__builtin_fma(d, d, E)));
        } else {
            Y_ = max_f64(Y_, y);
        }
        yp_ = y;
    };
    auto date = [&](int j, double z, double E) {
        W += z;
        const double yk = o.yk[j];
        side(fma_scalar_addend(W, sbx_v, yk), E, Y, yp);
        if (ANTI)
            side(fnma_scalar_addend(W, sbx_v, yk), E, Y_m, yp_m);
    };
    auto bridge = [&](uint32_t blk, double &E0, double &E1) {   // the two dates 2 blk, 2 blk + 1
        E0 = E1 = 0.0;
        if (CONT) {
            double u[2];
            gen.uniforms(w, c0, blk, 9u /*MC_DOMAIN_LOOKBACK_BRIDGE*/, u);
            E0 = neg2log_unit_tab(u[0], K), E1 = neg2log_unit_tab(u[1], K);
        }
    };
    int j = 0;
    if constexpr (Gen::cursor_phases > 1) {
#pragma unroll 1
        for (; j + 8 <= n; j += 8) {
            uint32_t blk = (uint32_t)(j >> 3);
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                // a pair's generator calls start after the running maximum of the pair before it: barrier_path<double>'s tie
                if (k)
                    asm("" : "+v"(Y), "+s"(blk));
                double z0, z1, E0, E1;
                gen.pair(w, c0, 8u /*MC_DOMAIN_LOOKBACK*/, (blk << 2) | k, carry, z0, z1);
                // ... and the pair's uniforms after its normals (the same tie): overlapped, the two generator calls and the mirrored
                // path's state need 131 vector registers, three waves per SIMD instead of four
                uint32_t ub = (blk << 2) | k;
                if (CONT)
                    asm("" : "+v"(z1), "+s"(ub));
                bridge(ub, E0, E1);
                date(j + 2 * (int)k, z0, E0);
                date(j + 2 * (int)k + 1, z1, E1);
            }
        }
    }
#pragma unroll 1
    for (; j < n; j += 2) {
        double z0, z1, E0, E1;
        gen.pair(w, c0, 8u /*MC_DOMAIN_LOOKBACK*/, (uint32_t)(j >> 1), carry, z0, z1);
        bridge((uint32_t)(j >> 1), E0, E1);
        date(j, z0, E0);
        if (j + 1 < n)   // wave-uniform
            date(j + 1, z1, E1);
    }
    gen.pairs_done((uint32_t)((n + 1) >> 1));
    double val = lookback_value(Y, yp, o);
    if (ANTI)
        val = 0.5 * (val + lookback_value(Y_m, yp_m, o));
    return val;
}

// one lane per path, grid-stride over the segment's paths: barrier_kernel's frame
template <class Real, bool ANTI, bool CONT, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void lookback_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const LookbackArgs<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = lookback_path<ANTI, CONT>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// Calls under Merton's jump-diffusion on m equally spaced dates: European, arithmetic-average and discretely monitored barrier
// (the model is stated in mc_mi355x.h).  Not in the reference.  The first walk here that is DISCONTINUOUS: date j draws, besides
// its normal z_j, a Poisson count N_j, and given N_j the diffusion plus the jumps of the date is ONE normal of deviation s_{N_j}:
//   C_j = C_{j-1} + N_j (a per-lane integer),   A_j = fma(s_{N_j}, z_j, A_{j-1}),   x_j = fma(C_j, emu, xk_j) + A_j
// with xk_j = ln S0 + j a from the per-date table (asian_path's: folded in fp64, rounded once, wave-uniform j: scalar loads).
// The count is an exact integer inversion of one raw Philox word wd against K wave-uniform thresholds T_0 <= ... <= T_{K-1}
// (scalar loads again, the compare's scalar operand): N = #{k : wd >= T_k}.  The thresholds are nondecreasing, so the hits of a
// lane are a prefix and the loop over k ends, for the whole wave, at the first k no lane reaches: a date on which no lane jumps
// costs ONE compare and a branch, and everything a jump needs sits behind that branch -- per trip of k one compare, one select
// s = hit ? s_{k+1} : s (a select chain: s_n is the host's fp64-folded value bit for bit, no root and no LDS gather on the
// device), one add C += hit; then one int-to-float conversion of C per jump date.
//   EUROPEAN: one exponential at maturity.  ASIAN: one per date, asian_path's.  BARRIER: barrier_path's running minimum of
//   d_j = fma(A_j, dsg, fma(C_j, dmu, dk_j)) in natural-log units (dk_j = sgn (ln B - ln S0 - j a), dsg = -sgn, dmu = -sgn mu_j),
//   P by a select, S_T = E(fma(A_m, ex, fma(C_m, emu, xT))).
//   ANTI: the same at -z on the SAME counts: A^- = -A exactly, so the mirrored path costs no state of its own beyond its sum / minimum.
// Stream: normals domain 10, the Asian layout; counts domain 11, raw Philox blocks of the same unit: fp32 date j (0-based here) =
// word j % 4 of block j / 4, fp64 date j = words 2 (j % 2), 2 (j % 2) + 1 of block j / 2 as (lo, hi).
// =========================================================================================
enum { MERTON_EUROPEAN = 0, MERTON_ASIAN = 1, MERTON_BARRIER = 2 };   // MC_MERTON_*
template <class Real> struct MertonWord;
template <> struct MertonWord<float> { using type = uint32_t; };
template <> struct MertonWord<double> { using type = uint64_t; };

template <class Real>
struct MertonArgs {
    const Real *xk;                                // n_dates values: xk_j in exponent units, or dk_j in natural-log units (barrier)
    const typename MertonWord<Real>::type *thr;    // n_thr thresholds
    const Real *sn;                                // n_thr + 1 values: s_0 ... s_K in the units of xk
    int n_dates, n_thr;
    typename MertonWord<Real>::type thr0;          // T_0 and s_0 once more, as kernel arguments: every date reads them
    Real s0;
    Real emu;         // mu_j in exponent units (natural log in f64, log2 in f32)
    Real dmu, dsg;    // barrier: -sgn mu_j and -sgn
    Real xT, ex;      // barrier: ln S_T = xT + emu C_m + ex A_m in exponent units
    Real strike;
    Real inv_m;       // 1 / n_dates
    Real c0, c1;      // barrier: value = (c0 + c1 P) payoff
};

// One date's count: s enters as s_0 and leaves as s_N, C grows by N, Cf follows C.  Every branch is wave-uniform.
template <class Real>
__device__ __forceinline__ void merton_count(const MertonArgs<Real> &o, typename MertonWord<Real>::type wd, Real &s, int &C, Real &Cf)
{
    if (o.n_thr <= 0)
        return;
    // the table is written before the launch and only read here: through the constant address space its loads are scalar loads
    // whatever hipcc can prove about the stores around them (inside this loop nest it gives up and emits masked vector loads)
    const auto *sn = (const __attribute__((address_space(4))) Real *)o.sn;
    const auto *thr = (const __attribute__((address_space(4))) typename MertonWord<Real>::type *)o.thr;
    bool hit = wd >= o.thr0;
    if (__builtin_amdgcn_ballot_w64(hit) == 0)
        return;
    int k = 0;
#pragma unroll 1
    do {
        ++k;
        const Real sk = sn[k];   // taken whether or not a lane selects it: a scalar load and the select's scalar operand
        s = hit ? sk : s;
        C += hit ? 1 : 0;
        if (k >= o.n_thr)
            break;
        hit = wd >= thr[k];
    } while (__builtin_amdgcn_ballot_w64(hit) != 0);
    Cf = (Real)C;
}

template <int PAYOFF, class Real>
__device__ __forceinline__ Real merton_value(Real A, Real Cf, Real sum, Real mn, const MertonArgs<Real> &o)
{
    if (PAYOFF == MERTON_ASIAN) {
        const Real a = fma_r(sum, o.inv_m, -o.strike);
        return a > 0 ? a : 0;
    }
    if (PAYOFF == MERTON_BARRIER) {
        const Real P = mn > 0 ? (Real)1 : (Real)0;   // the select
        const Real pay = exp_model(fma_r(A, o.ex, fma_r(Cf, o.emu, o.xT))) - o.strike;
        return fma_r(o.c1, P, o.c0) * (pay > 0 ? pay : 0);
    }
    const Real pay = exp_model(fma_r(Cf, o.emu, o.xk[o.n_dates - 1]) + A) - o.strike;
    return pay > 0 ? pay : 0;
}

// fp32: four dates per trip, one block of normals and one raw block of count words.
template <bool ANTI, int PAYOFF, class Gen>
__device__ __forceinline__ float merton_path(Gen &gen, const MertonArgs<float> &o, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<float>();
    static_assert(NPB == 4, "four dates per block of normals and per block of words");
    const int n = o.n_dates;
    float A = 0, Cf = 0, sum = 0, sum_m = 0, mn = __builtin_inff(), mn_m = __builtin_inff();
    int C = 0;
    float z[NPB];
    auto date = [&](int j, float zj, uint32_t wd) {
        float s = o.s0;
        merton_count(o, wd, s, C, Cf);
        A = __builtin_fmaf(s, zj, A);
        if (PAYOFF == MERTON_ASIAN) {
            const float base = __builtin_fmaf(Cf, o.emu, o.xk[j]);
            sum += __builtin_amdgcn_exp2f(base + A);
            if (ANTI)
                sum_m += __builtin_amdgcn_exp2f(base - A);
        }
        if (PAYOFF == MERTON_BARRIER) {
            const float base = __builtin_fmaf(Cf, o.dmu, o.xk[j]);
            mn = __builtin_fminf(mn, __builtin_fmaf(A, o.dsg, base));
            if (ANTI)
                mn_m = __builtin_fminf(mn_m, __builtin_fmaf(-A, o.dsg, base));
        }
    };
    int j0 = 0;
    for (; j0 + NPB <= n; j0 += NPB) {
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 10u /*MC_DOMAIN_MERTON*/, z);
        const u32x4 r = gen.words(w, c0, (uint32_t)(j0 / NPB), 11u /*MC_DOMAIN_MERTON_JUMPS*/);
        date(j0, z[0], r.x);
        date(j0 + 1, z[1], r.y);
        date(j0 + 2, z[2], r.z);
        date(j0 + 3, z[3], r.w);
    }
    if (j0 < n) {   // wave-uniform: one to three dates left
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 10u /*MC_DOMAIN_MERTON*/, z);
        const u32x4 r = gen.words(w, c0, (uint32_t)(j0 / NPB), 11u /*MC_DOMAIN_MERTON_JUMPS*/);
        date(j0, z[0], r.x);
        if (j0 + 1 < n)
            date(j0 + 1, z[1], r.y);
        if (j0 + 2 < n)
            date(j0 + 2, z[2], r.z);
    }
    float val = merton_value<PAYOFF>(A, Cf, sum, mn, o);
    if (ANTI)
        val = 0.5f * (val + merton_value<PAYOFF>(-A, Cf, sum_m, mn_m, o));
    return val;
}

// fp64: asian_path<double>'s loop (Box-Muller pairs through the generator's pair cursor, four pairs per trip, then one); a pair of
// dates takes its two 64-bit count words from one raw Philox block.  emu (dmu) sits in a vector register for the whole path, so
// the date's fma reads xk_j from its SGPR pair; the running minimum is min_f64.
template <bool ANTI, int PAYOFF, class Gen>
__device__ __forceinline__ double merton_path(Gen &gen, const MertonArgs<double> &o, const Work &w, uint32_t c0)
{
    const int n = o.n_dates;
    double A = 0, Cf = 0, sum = 0, sum_m = 0, mn = __builtin_inf(), mn_m = __builtin_inf();
    int C = 0;
    [[maybe_unused]] const double mu_v = to_vgpr(PAYOFF == MERTON_BARRIER ? o.dmu : o.emu);
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    auto date = [&](int j, double zj, uint32_t lo, uint32_t hi) {
        double s = o.s0;
        merton_count(o, ((uint64_t)hi << 32) | lo, s, C, Cf);
        A = __builtin_fma(s, zj, A);
        if (PAYOFF == MERTON_ASIAN) {
            const double base = fma_scalar_addend(Cf, mu_v, o.xk[j]);
            sum += exp_f64(base + A);
            if (ANTI)
                sum_m += exp_f64(base - A);
        }
        if (PAYOFF == MERTON_BARRIER) {
            const double base = fma_scalar_addend(Cf, mu_v, o.xk[j]);
            mn = min_f64(mn, __builtin_fma(A, o.dsg, base));
            if (ANTI)
                mn_m = min_f64(mn_m, __builtin_fma(-A, o.dsg, base));
        }
    };
    int j = 0;
    if constexpr (Gen::cursor_phases > 1) {
#pragma unroll 1
        for (; j + 8 <= n; j += 8) {
            uint32_t blk = (uint32_t)(j >> 3);
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                // a pair's generator calls start after the walk (and the sums) of the pair before it, and its count words after its
                // normals: barrier_path<double>'s tie.  Left free, hipcc overlaps the eight exponentials of a trip
                if (k)
                    asm("" : "+v"(A), "+v"(sum), "+v"(sum_m), "+s"(blk));
                double z0, z1;
                gen.pair(w, c0, 10u /*MC_DOMAIN_MERTON*/, (blk << 2) | k, carry, z0, z1);
                uint32_t ub = (blk << 2) | k;
                asm("" : "+v"(z1), "+s"(ub));
                const u32x4 r = gen.words(w, c0, ub, 11u /*MC_DOMAIN_MERTON_JUMPS*/);
                date(j + 2 * (int)k, z0, r.x, r.y);
                if (PAYOFF == MERTON_ASIAN)   // the second date's exponentials after the first's
                    asm("" : "+v"(A), "+v"(sum), "+v"(sum_m));
                date(j + 2 * (int)k + 1, z1, r.z, r.w);
            }
        }
    }
#pragma unroll 1
    for (; j < n; j += 2) {
        double z0, z1;
        gen.pair(w, c0, 10u /*MC_DOMAIN_MERTON*/, (uint32_t)(j >> 1), carry, z0, z1);
        const u32x4 r = gen.words(w, c0, (uint32_t)(j >> 1), 11u /*MC_DOMAIN_MERTON_JUMPS*/);
        date(j, z0, r.x, r.y);
        if (j + 1 < n)   // wave-uniform
            date(j + 1, z1, r.z, r.w);
    }
    gen.pairs_done((uint32_t)((n + 1) >> 1));
    double val = merton_value<PAYOFF>(A, Cf, sum, mn, o);
    if (ANTI)
        val = 0.5 * (val + merton_value<PAYOFF>(-A, Cf, sum_m, mn_m, o));
    return val;
}

// one lane per path, grid-stride over the segment's paths: asian_kernel's frame
template <class Real, bool ANTI, int PAYOFF, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void merton_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const MertonArgs<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = merton_path<ANTI, PAYOFF>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// Bermudan put / call on m equally spaced exercise dates under a GIVEN exercise rule: the pricing pass of Longstaff-Schwartz
// (the model is stated in mc_mi355x.h).  Not in the reference.  The walk is asian_path's -- W_j = z_1 + ... + z_j the lane's
// only state of the walk, x_j = fma(W_j, bx, xk_j) in units of the strike -- and date j's ROW of six wave-uniform values
//   xk_j = ln(s/k) + j a (exponent units),  g_j = exp(r (t - t_j)),  beta_j0 .. beta_j3
// comes from the per-date table (folded in fp64, rounded once) through scalar loads.  A date costs one exponential, the payoff
// p = max(q (e - 1), 0), three fmas of Horner C = ((b3 p + b2) p + b1) p + b0, one multiply p g, two compares and a select:
//   ex = p > 0 && p g > C;   value = alive && ex ? p g : value;   alive &= !ex
// alive is a lane mask: and-ed on the scalar unit.  The LAST date's row is written by the host as {-inf, 0, 0, 0}: p g > -inf
// holds for every p > 0, so "exercise iff p_m > 0" needs no code of its own; a never-exercise row is {+inf, 0, 0, 0}.  With
// b1 = b2 = b3 = 0 the Horner form passes +-inf through without a NaN for every finite p.
//   ANTI: the same at -W, with its own mask and value; the mean of the two.
// The walk always runs to maturity, also when no lane of the wave is alive any more: see DESIGN 4.13.
// Stream: domain 12, the Asian layout.
// =========================================================================================
enum { AMERICAN_ROW = 6 };   // values per date in the table
template <class Real>
struct AmericanArgs {
    const Real *rows;   // n_dates rows {xk, g, b0, b1, b2, b3}
    int n_dates;
    Real bx;            // v sqrt(dt) in exponent units
    Real q;             // -1 put, +1 call
};

// Payoff, continuation value and decision of one date at the spot e (in units of the strike): what a fit of the rule and the
// pricing pass must agree on to the bit.  pg = p g, the path's value if it exercises here.
template <class Real>
__device__ __forceinline__ bool american_decide(Real e, Real q, Real g, Real b0, Real b1, Real b2, Real b3, Real &pg)
{
    const Real d = fma_r(e, q, -q);
    const Real p = d > 0 ? d : 0;
    const Real C = fma_r(fma_r(fma_r(b3, p, b2), p, b1), p, b0);
    pg = p * g;
    return p > 0 && pg > C;
}

// the date's row through the constant address space: the table is written before the launch and only read here, and its loads
// must be scalar loads whatever hipcc can prove about the stores around them (merton_count's remedy)
template <class Real> using AmericanRowPtr = const __attribute__((address_space(4))) Real *;

template <bool ANTI, class Real>
__device__ __forceinline__ void american_date(AmericanRowPtr<Real> r, Real q, Real x, Real x_m, bool &alive, bool &alive_m, Real &val, Real &val_m)
{
    const Real g = r[1], b0 = r[2], b1 = r[3], b2 = r[4], b3 = r[5];
    Real pg;
    const bool ex = american_decide(exp_model(x), q, g, b0, b1, b2, b3, pg);
    val = alive && ex ? pg : val;
    alive = alive && !ex;
    if (ANTI) {
        const bool ex_m = american_decide(exp_model(x_m), q, g, b0, b1, b2, b3, pg);
        val_m = alive_m && ex_m ? pg : val_m;
        alive_m = alive_m && !ex_m;
    }
}

// fp32: four dates per trip, one Philox block.
template <bool ANTI, class Gen>
__device__ __forceinline__ float american_path(Gen &gen, const AmericanArgs<float> &o, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<float>();
    static_assert(NPB == 4, "four dates per block");
    const auto rows = (AmericanRowPtr<float>)o.rows;
    const int n = o.n_dates;
    float W = 0, val = 0, val_m = 0;
    bool alive = true, alive_m = true;
    float z[NPB];
    auto date = [&](int j, float zj) {
        W += zj;
        const auto r = rows + AMERICAN_ROW * j;
        const float xk = r[0];
        american_date<ANTI>(r, o.q, __builtin_fmaf(W, o.bx, xk), __builtin_fmaf(-W, o.bx, xk), alive, alive_m, val, val_m);
    };
    int j0 = 0;
    for (; j0 + NPB <= n; j0 += NPB) {
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 12u /*MC_DOMAIN_AMERICAN*/, z);
        date(j0, z[0]);
        date(j0 + 1, z[1]);
        date(j0 + 2, z[2]);
        date(j0 + 3, z[3]);
    }
    if (j0 < n) {   // wave-uniform: one to three dates left
        gen.normals(w, c0, (uint32_t)(j0 / NPB), 12u /*MC_DOMAIN_AMERICAN*/, z);
        date(j0, z[0]);
        if (j0 + 1 < n)
            date(j0 + 1, z[1]);
        if (j0 + 2 < n)
            date(j0 + 2, z[2]);
    }
    return ANTI ? 0.5f * (val + val_m) : val;
}

// fp64: asian_path<double>'s loop (Box-Muller pairs through the generator's pair cursor, four pairs per trip, then one).  bx (and
// -bx for the mirrored path) sit in vector registers for the whole path, so x = fma(W, bx, xk_j) reads xk_j from its SGPR pair.
template <bool ANTI, class Gen>
__device__ __forceinline__ double american_path(Gen &gen, const AmericanArgs<double> &o, const Work &w, uint32_t c0)
{
    const auto rows = (AmericanRowPtr<double>)o.rows;
    const int n = o.n_dates;
    double W = 0, val = 0, val_m = 0;
    bool alive = true, alive_m = true;
    const double bx_v = to_vgpr(o.bx);
    [[maybe_unused]] const double nbx_v = to_vgpr(-o.bx);
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    auto date = [&](int j, double zj) {
        W += zj;
        const auto r = rows + AMERICAN_ROW * j;
        const double xk = r[0];
        american_date<ANTI>(r, o.q, fma_scalar_addend(W, bx_v, xk), ANTI ? fma_scalar_addend(W, nbx_v, xk) : 0.0, alive, alive_m, val, val_m);
    };
    auto tie = [&](uint32_t &blk) {
        if constexpr (ANTI)
            asm("" : "+v"(W), "+v"(val), "+v"(val_m), "+s"(blk));
        else
            asm("" : "+v"(W), "+v"(val), "+s"(blk));
    };
    int j = 0;
    if constexpr (Gen::cursor_phases > 1) {
#pragma unroll 1
        for (; j + 8 <= n; j += 8) {
            uint32_t blk = (uint32_t)(j >> 3);
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                // a pair's generator call starts after the walk of the pair before it (barrier_path<double>'s tie): left free, hipcc
                // overlaps the exponentials of a trip and hoists the eight rows' scalar loads to its top (131 VGPRs, 21 SGPR spills)
                if (k)
                    tie(blk);
                double z0, z1;
                gen.pair(w, c0, 12u /*MC_DOMAIN_AMERICAN*/, (blk << 2) | k, carry, z0, z1);
                const int jd = (int)(blk << 3) + 2 * (int)k;   // the rows' addresses hang on the tie: their scalar loads stay behind it
                date(jd, z0);
                tie(blk);   // the second date's exponential after the first's
                date(jd + 1, z1);
            }
        }
    }
#pragma unroll 1
    for (; j < n; j += 2) {
        double z0, z1;
        gen.pair(w, c0, 12u /*MC_DOMAIN_AMERICAN*/, (uint32_t)(j >> 1), carry, z0, z1);
        date(j, z0);
        if (j + 1 < n)   // wave-uniform
            date(j + 1, z1);
    }
    gen.pairs_done((uint32_t)((n + 1) >> 1));
    return ANTI ? 0.5 * (val + val_m) : val;
}

// one lane per path, grid-stride over the segment's paths: asian_kernel's frame
template <class Real, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void american_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const AmericanArgs<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = american_path<ANTI>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// The Longstaff-Schwartz FIT of that rule: the first product here whose paths are not independent -- a date's rule is a regression
// over all paths -- so the fit is one launch per date, j = m ... 0, with the per-path state (W, V) in global memory between them.
// The walk runs BACKWARD without storing the path: W_m = sqrt(m) z_m, W_j = j/(j+1) W_{j+1} + sqrt(j/(j+1)) z_j is the Brownian
// bridge from 0, exact in law (the host passes cw = j/(j+1), cz = sqrt(j/(j+1)); j = m: cw = 0, cz = sqrt(m)).  Launch j, lane = path:
//   load (W_{j+1}, V);  j + 1 < m: apply date j + 1's decision with row j + 1 of the device table (american_decide, the pricing
//   pass's own), V = ex ? p g : V;  draw z_j, step to W_j, p_j = payoff at W_j;  j = m: V = p_m;  store (W_j, V);
//   0 < j < m and p_j > 0: add p_j^k, k = 0 .. 6, and p_j^k V, k = 0 .. 3, in fp64;   j = 0: add V and V^2.
// The twelve sums leave as six (s, q) pairs, one per plane of the call's pair buffer, the way vanilla_greeks_kernel's do; the last
// workgroup writes them as six triples {sums[2 i], sums[2 i + 1], n}.  american_solve_kernel, one lane between two date launches,
// reads them, solves the date's normal equations (mc_american_solve's arithmetic, operation for operation, contraction off) and writes row
// j of the table, rounded once to Real, and an fp64 copy for the host: all 2 m + 1 launches go on the stream without a host
// synchronisation in between.  Stream: domain 13, the Asian layout (a date draws one entry of its block; the rest is dead code).
// =========================================================================================
enum { AMERICAN_FIT_PLANES = 6 };
template <class Real>
struct AmericanFitArgs {
    Real *W, *V;         // the state of the launch's first path
    const Real *rows;    // the device table: n_dates rows {xk, g, b0 .. b3}; american_solve_kernel writes the b's
    int j, n_dates;      // the date this launch walks TO
    Real bx, q;
    Real cw, cz;         // W_j = cw W_{j+1} + cz z_j
};

template <class Real, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void american_fit_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const AmericanFitArgs<Real> o, const Work w)
{
    stage_tables<Real>();
    constexpr int NPB = Gen::template npb<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc[2 * AMERICAN_FIT_PLANES] = {};
    Gen gen(w);
    const auto rows = (AmericanRowPtr<Real>)o.rows;
    const int j = o.j, m = o.n_dates;   // wave-uniform: every branch on them is a scalar branch
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        Real W = 0, V = 0;
        if (j < m) {
            W = o.W[i], V = o.V[i];
            if (j + 1 < m) {   // date j + 1's decision, with the rule the solve between the two launches wrote
                const auto r = rows + AMERICAN_ROW * j;
                Real pg;
                const bool ex = american_decide(exp_model(fma_r(W, o.bx, r[0])), o.q, r[1], r[2], r[3], r[4], r[5], pg);
                V = ex ? pg : V;
            }
        }
        if (j == 0) {
            pair_add(acc, 0, (double)V);
            continue;
        }
        Real z[NPB];
        gen.normals(w, w.unit_lo + i, (uint32_t)(j - 1) / NPB, 13u /*MC_DOMAIN_AMERICAN_FIT*/, z);
        Real zj = z[0];
#pragma unroll
        for (int e = 1; e < NPB; ++e)   // a select chain on a wave-uniform index: no indexed register array
            zj = (j - 1) % NPB == e ? z[e] : zj;
        W = fma_r(o.cw, W, o.cz * zj);
        const Real d = fma_r(exp_model(fma_r(W, o.bx, rows[AMERICAN_ROW * (j - 1)])), o.q, -o.q);
        const Real p = d > 0 ? d : 0;
        if (j == m)
            V = p;
        o.W[i] = W, o.V[i] = V;
        if (j < m && p > 0) {
            const double p1 = (double)p, v = (double)V, p2 = p1 * p1, p3 = p2 * p1;
            acc[0] += 1.0, acc[1] += p1, acc[2] += p2, acc[3] += p3, acc[4] += p2 * p2, acc[5] += p2 * p3, acc[6] += p3 * p3;
            acc[7] += v, acc[8] += p1 * v, acc[9] += p2 * v, acc[10] += p3 * v;
        }
    }
#pragma unroll
    for (int q = 0; q < AMERICAN_FIT_PLANES; ++q) {
        group_sum2(acc[2 * q], acc[2 * q + 1]);
        pair_publish(late_tail(acc[2 * q]), acc, q, q);
    }
    arrive_and_finish(late_tail(acc[0]));
}

// sums[i] of mc_american_solve from the six triples of a date launch
__device__ __forceinline__ double american_sum(const double *triples, int i) { return triples[3 * (i >> 1) + (i & 1)]; }

// One lane.  mc_american_solve (mc_hostmath.c) restated for the device, operation for operation, with contraction off.  Equal bits
// with the host are not claimed: that would also need the device's fp64 division and root correctly rounded, and no test feeds one
// set of sums through both (the whole fit is compared with the float64 model within 16 times the model's own movement).
template <class Real, int DEGREE>
__global__ void american_solve_kernel(const double *__restrict__ triples, Real *__restrict__ row_beta, double *__restrict__ beta64)
{
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    constexpr int N = DEGREE + 1;
    double beta[4] = {__builtin_inf(), 0.0, 0.0, 0.0};
    double d[N], l[N][N], y[N];
    bool ok = american_sum(triples, 0) >= 32.0 /*MC_AMERICAN_MIN_ITM*/;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double a = american_sum(triples, 2 * i);
        ok = ok && a > 0 && a < __builtin_inf();
        d[i] = __builtin_sqrt(ok ? a : 1.0);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int k = 0; k <= i; ++k) {
            double a = american_sum(triples, i + k) / (d[i] * d[k]);
#pragma unroll
            for (int c = 0; c < k; ++c)
                a -= l[i][c] * l[k][c];
            if (k < i) {
                l[i][k] = a / l[k][k];
            } else {
                ok = ok && a > 0;
                l[i][i] = __builtin_sqrt(ok ? a : 1.0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double a = american_sum(triples, 7 + i) / d[i];
#pragma unroll
        for (int c = 0; c < i; ++c)
            a -= l[i][c] * y[c];
        y[i] = a / l[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double a = y[i];
#pragma unroll
        for (int c = i + 1; c < N; ++c)
            a -= l[c][i] * y[c];
        y[i] = a / l[i][i];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        y[i] = y[i] / d[i];
        ok = ok && __builtin_fabs(y[i]) < __builtin_inf();
    }
    if (ok) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            beta[i] = y[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        row_beta[i] = (Real)beta[i];
        beta64[i] = beta[i];
    }
}

// =========================================================================================
// European call under the Heston stochastic-volatility model, full-truncation Euler in log space on m equal steps (the model
// is stated in mc_mi355x.h).  Not in the reference.  The first walk here whose step is non-linear in its state: besides the
// normals a lane carries the variance V and two running sums, because
//   x_m = ln S0 + r T - (dt/2) sum_j V+_{j-1} + sdt sum_j s_{j-1} z1_j          (V+ = max(V, 0), s = sqrt(V+))
// is the same real number as the step-by-step x_j and leaves two accumulations per step; the exponential is taken once, at
// maturity.  Per step, with t = c1 z1 + c2 z2 (c1 = xi sdt rho, c2 = xi sdt rho'):
//   V+ = max(V, 0);  s = sqrt(V+);  sv += V+;  sw = fma(s, z1, sw);  V = fma(s, t, fma(-kdt, V+, V + ktdt))
// Every constant is a kernel argument, folded on the host in fp64 and rounded once: no table.
//   ANTI: a second (V, sv, sw) walked on (-z1, -z2) -- nothing is shared but the normals and t -- value = mean of the two
// sqrt(0) on a truncated step: fp32 takes v_sqrt_f32, which gives 0 exactly; fp64 takes sqrt_trunc below.
// Stream: domain 6, step j (0-based here) = entries 2j % NPB, 2j % NPB + 1 of block 2j / NPB: fp32 two steps per Philox
// block, fp64 pair j of the pair cursor.
// =========================================================================================
template <class Real>
struct HestonArgs {
    int n_steps;
    Real v0;
    Real kdt, ktdt;   // kappa dt, kappa theta dt
    Real c1, c2;      // xi sqrt(dt) rho, xi sqrt(dt) sqrt(1 - rho^2)
    Real x0, av, aw;  // x_m = x0 + av sum V+ + aw sum s z1 in exponent units (natural log in f64, log2 in f32): ln S0 + r T, -dt/2, sqrt(dt)
    Real strike;
};

template <class Real>
struct HestonSide {
    Real V, sv, sw;   // the variance, sum V+, sum s z1
};

__device__ __forceinline__ float sqrt_trunc(float, float vp, float) { return __builtin_amdgcn_sqrtf(vp); }
__device__ __forceinline__ float max0(float v) { return __builtin_fmaxf(v, 0.0f); }
// max(a, 0) and max(a, b) of doubles that are never signalling NaNs as ONE v_max_f64 each (see min_f64)
__device__ __forceinline__ double max0(double a)
{
    double r;
    asm("v_max_f64 %0, %1, 0" : "=v"(r) : "v"(a));
    return r;
}
__device__ __forceinline__ double max_scalar_f64(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(b));
    return r;
}
// sqrt(max(v, 0)) in fp64, vp = max(v, 0) given.  sqrt_pos (mc_math_f64.hpp) starts from v_rsq_f64 of the radicand, which is inf at
// 0 and makes inf * 0 of a truncated step.  Here the reciprocal root is taken of max(v, floor), floor = 2^-1000, and multiplied
// into vp: at vp = 0 every product below is an exact 0 next to finite factors and the result is exactly 0; for 0 < vp < floor
// the Newton steps do not converge, but everything stays below 2^-498 and so does the error; from floor up it is sqrt_pos
// instruction for instruction.  Cost: one v_max_f64 per root, no compare, no select.
__device__ __forceinline__ double sqrt_trunc(double v, double vp, double floor)
{
    const double y = __builtin_amdgcn_rsq(max_scalar_f64(v, floor));
    double g = vp * y;
    double h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    const double d = __builtin_fma(-g, g, vp);
    return __builtin_fma(d, h, g);
}

template <class Real>
__device__ __forceinline__ void heston_step(HestonSide<Real> &p, Real z1, Real t, const HestonArgs<Real> &o, Real floor)
{
    const Real vp = max0(p.V);
    const Real s = sqrt_trunc(p.V, vp, floor);
    p.sv += vp;
    p.sw = fma_r(s, z1, p.sw);
    p.V = fma_r(s, t, fma_r(-o.kdt, vp, p.V + o.ktdt));
}

template <class Real>
__device__ __forceinline__ Real heston_value(const HestonSide<Real> &p, const HestonArgs<Real> &o)
{
    const Real pay = exp_model(fma_r(o.aw, p.sw, fma_r(o.av, p.sv, o.x0))) - o.strike;
    return pay > 0 ? pay : 0;
}

// fp32: one Philox block of four normals = two steps per trip
template <bool ANTI, class Gen>
__device__ __forceinline__ float heston_path(Gen &gen, const HestonArgs<float> &o, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<float>();
    static_assert(NPB == 4, "two steps per block");
    const int n = o.n_steps;
    HestonSide<float> p = {o.v0, 0.0f, 0.0f}, q = p;
    float z[NPB];
    auto step = [&](float z1, float z2) {
        const float t = __builtin_fmaf(z2, o.c2, o.c1 * z1);
        heston_step(p, z1, t, o, 0.0f);
        if (ANTI)
            heston_step(q, -z1, -t, o, 0.0f);
    };
    int j = 0;
    for (; j + 2 <= n; j += 2) {
        gen.normals(w, c0, (uint32_t)(j >> 1), 6u /*MC_DOMAIN_HESTON*/, z);
        step(z[0], z[1]);
        step(z[2], z[3]);
    }
    if (j < n) {   // wave-uniform: the odd last step
        gen.normals(w, c0, (uint32_t)(j >> 1), 6u /*MC_DOMAIN_HESTON*/, z);
        step(z[0], z[1]);
    }
    float val = heston_value(p, o);
    if (ANTI)
        val = 0.5f * (val + heston_value(q, o));
    return val;
}

// fp64: one Box-Muller pair of the generator's pair cursor per step, four pairs per trip for the bulk (the cursor's phase a
// compile-time constant in each copy), one pair per trip for the rest: asian_path<double>'s loop with a step where it has two dates.
template <bool ANTI, class Gen>
__device__ __forceinline__ double heston_path(Gen &gen, const HestonArgs<double> &o, const Work &w, uint32_t c0)
{
    const int n = o.n_steps;
    HestonSide<double> p = {o.v0, 0.0, 0.0}, q = p;
    const double floor = 0x1p-1000;
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    auto step = [&](double z1, double z2) {
        const double t = __builtin_fma(z2, o.c2, o.c1 * z1);
        heston_step(p, z1, t, o, floor);
        if (ANTI)
            heston_step(q, -z1, -t, o, floor);
    };
    int j = 0;
    if constexpr (Gen::cursor_phases > 1) {
#pragma unroll 1
        for (; j + 4 <= n; j += 4) {
            uint32_t g4 = (uint32_t)(j >> 2) << 2;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                // a step's generator call starts after the variance of the step before it (its pair index passes through the same
                // empty statement: barrier_path<double>'s tie).  Left free, hipcc overlaps the four calls of a trip around the few
                // instructions of the steps and the antithetic form needs 132 vector registers: three waves per SIMD instead of four.
                if (ANTI && k)
                    asm("" : "+v"(p.V), "+s"(g4));
                double z0, z1;
                gen.pair(w, c0, 6u /*MC_DOMAIN_HESTON*/, g4 | k, carry, z0, z1);
                step(z0, z1);
            }
        }
    }
#pragma unroll 1
    for (; j < n; ++j) {
        double z0, z1;
        gen.pair(w, c0, 6u /*MC_DOMAIN_HESTON*/, (uint32_t)j, carry, z0, z1);
        step(z0, z1);
    }
    gen.pairs_done((uint32_t)n);
    double val = heston_value(p, o);
    if (ANTI)
        val = 0.5 * (val + heston_value(q, o));
    return val;
}

// one lane per path, grid-stride over the segment's paths
template <class Real, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void heston_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const HestonArgs<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = heston_path<ANTI>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// Path-dependent calls on the Heston walk above: the arithmetic-average call (PAYOFF = 0) and the single-barrier call
// monitored on the dates (PAYOFF = 1).  Not in the reference.  The walk takes n_steps = n_dates * steps_per_date steps of
// heston_step; date d (1-based) falls after step d * steps_per_date and reads the log price from the two running sums:
//   Asian:    x_d = fma(aw, sw, fma(av, sv, xk_d)),   xk_d = ln S0 + r t_d in exponent units;  sum S += E(x_d)
//   barrier:  d_d = fma(aw, sw, fma(av, sv, dk_d)),   dk_d = sgn (ln B - ln S0 - r t_d), (av, aw) = sgn (dt/2, -sdt), natural-log
//             units; mn = min(mn, d_d);  P = [mn > 0] by a select;  value = (c0 + c1 P) heston_value (the one exponential)
// The date's addend comes from the context's constant table (one value per date, folded in fp64 and rounded once) through
// scalar loads: the date index is wave-uniform, and so is the countdown to the next date -- both live in SGPRs, the date's
// code sits behind a scalar branch, and the steps between two dates are heston_path's.
//   ANTI: a second walk on (-z1, -z2) with its own sums and its own running average / minimum; value = mean of the two
// Stream: domain 7, the Heston layout.  Continuous monitoring is not offered: the Brownian-bridge factor of barrier_kernel
// assumes a constant variance between two dates.
// =========================================================================================
template <class Real>
struct HestonPathArgs {
    HestonArgs<Real> h;   // the walk; (x0, av, aw, strike) give the value at maturity
    const Real *tab;      // n_dates values: xk_d (Asian) or dk_d (barrier)
    int steps_per_date;
    Real av, aw;          // the date's coefficients of sum V+ and sum s z1
    Real inv_m;           // Asian: 1 / n_dates
    Real c0, c1;          // barrier: value = (c0 + c1 P) payoff
};

// what a path direction carries besides its HestonSide: sum S over the dates (Asian) or the running minimum distance (barrier)
template <int PAYOFF, class Real>
__device__ __forceinline__ Real heston_date_start()
{
    return PAYOFF == 0 ? (Real)0 : (Real)__builtin_inf();
}

__device__ __forceinline__ float min_r(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double min_r(double a, double b) { return min_f64(a, b); }

template <int PAYOFF, class Real>
__device__ __forceinline__ void heston_date(const HestonSide<Real> &p, Real &acc, Real addend, const HestonPathArgs<Real> &o)
{
    const Real x = fma_r(o.aw, p.sw, fma_r(o.av, p.sv, addend));
    if (PAYOFF == 0)
        acc += exp_model(x);
    else
        acc = min_r(acc, x);
}

template <int PAYOFF, class Real>
__device__ __forceinline__ Real heston_path_value(const HestonSide<Real> &p, Real acc, const HestonPathArgs<Real> &o)
{
    if (PAYOFF == 0) {
        const Real a = fma_r(acc, o.inv_m, -o.h.strike);
        return a > 0 ? a : 0;
    }
    const Real P = acc > 0 ? (Real)1 : (Real)0;   // the select, as barrier_value
    return fma_r(o.c1, P, o.c0) * heston_value(p, o.h);
}

// fp32: heston_path<float>'s trips, one Philox block = two steps.  After each step the scalar countdown `left` decides whether a
// date falls there: an odd steps_per_date puts one between the two steps of a block, which is the first of the two branches
// below and needs no second generator call.  n_steps is a multiple of steps_per_date, so the odd last step ends on a date.
template <bool ANTI, int PAYOFF, class Gen>
__device__ __forceinline__ float heston_path_walk(Gen &gen, const HestonPathArgs<float> &o, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<float>();
    static_assert(NPB == 4, "two steps per block");
    const int n = o.h.n_steps;
    HestonSide<float> p = {o.h.v0, 0.0f, 0.0f}, q = p;
    float acc = heston_date_start<PAYOFF, float>(), acc_m = acc;
    float z[NPB];
    auto step = [&](float z1, float z2) {
        const float t = __builtin_fmaf(z2, o.h.c2, o.h.c1 * z1);
        heston_step(p, z1, t, o.h, 0.0f);
        if (ANTI)
            heston_step(q, -z1, -t, o.h, 0.0f);
    };
    int d = 0, left = o.steps_per_date;
    auto date = [&]() {
        const float addend = o.tab[d];
        heston_date<PAYOFF>(p, acc, addend, o);
        if (ANTI)
            heston_date<PAYOFF>(q, acc_m, addend, o);
        ++d;
        left = o.steps_per_date;
    };
    int j = 0;
    for (; j + 2 <= n; j += 2) {
        gen.normals(w, c0, (uint32_t)(j >> 1), 7u /*MC_DOMAIN_HESTON_PATH*/, z);
        step(z[0], z[1]);
        if (--left == 0)   // wave-uniform
            date();
        step(z[2], z[3]);
        if (--left == 0)
            date();
    }
    if (j < n) {   // wave-uniform: the odd last step, which is the last date
        gen.normals(w, c0, (uint32_t)(j >> 1), 7u /*MC_DOMAIN_HESTON_PATH*/, z);
        step(z[0], z[1]);
        date();
    }
    float val = heston_path_value<PAYOFF>(p, acc, o);
    if (ANTI)
        val = 0.5f * (val + heston_path_value<PAYOFF>(q, acc_m, o));
    return val;
}

// fp64: heston_path<double>'s trips (four pairs per trip, then one), the same countdown after every step.
template <bool ANTI, int PAYOFF, class Gen>
__device__ __forceinline__ double heston_path_walk(Gen &gen, const HestonPathArgs<double> &o, const Work &w, uint32_t c0)
{
    const int n = o.h.n_steps;
    HestonSide<double> p = {o.h.v0, 0.0, 0.0}, q = p;
    double acc = heston_date_start<PAYOFF, double>(), acc_m = acc;
    const double floor = 0x1p-1000;
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    auto step = [&](double z1, double z2) {
        const double t = __builtin_fma(z2, o.h.c2, o.h.c1 * z1);
        heston_step(p, z1, t, o.h, floor);
        if (ANTI)
            heston_step(q, -z1, -t, o.h, floor);
    };
    int d = 0, left = o.steps_per_date;
    auto date = [&]() {
        const double addend = o.tab[d];
        heston_date<PAYOFF>(p, acc, addend, o);
        if (ANTI)
            heston_date<PAYOFF>(q, acc_m, addend, o);
        ++d;
        left = o.steps_per_date;
    };
    int j = 0;
    if constexpr (Gen::cursor_phases > 1) {
#pragma unroll 1
        for (; j + 4 <= n; j += 4) {
            uint32_t g4 = (uint32_t)(j >> 2) << 2;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                // heston_path<double>'s tie: a step's generator call starts after the variance of the step before it
                if (ANTI && k)
                    asm("" : "+v"(p.V), "+s"(g4));
                double z0, z1;
                gen.pair(w, c0, 7u /*MC_DOMAIN_HESTON_PATH*/, g4 | k, carry, z0, z1);
                step(z0, z1);
                if (--left == 0)   // wave-uniform
                    date();
            }
        }
    }
#pragma unroll 1
    for (; j < n; ++j) {
        double z0, z1;
        gen.pair(w, c0, 7u /*MC_DOMAIN_HESTON_PATH*/, (uint32_t)j, carry, z0, z1);
        step(z0, z1);
        if (--left == 0)
            date();
    }
    gen.pairs_done((uint32_t)n);
    double val = heston_path_value<PAYOFF>(p, acc, o);
    if (ANTI)
        val = 0.5 * (val + heston_path_value<PAYOFF>(q, acc_m, o));
    return val;
}

// one lane per path, grid-stride over the segment's paths
template <class Real, bool ANTI, int PAYOFF, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void heston_path_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const HestonPathArgs<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = heston_path_walk<ANTI, PAYOFF>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// One level of a multilevel estimator on the Heston walk: Y = P_fine - P_coarse, P the Asian payoff of heston_path_kernel (one date:
// the European call).  Not in the reference.  A lane walks the fine path on m steps of dt and the coarse path on m / 2 steps of
// 2 dt on the SAME Brownian increments, the normals drawn once: with the fine steps 2i - 1 and 2i of coarse step i,
//   W1 = z1_a + z1_b,  T = t_a + t_b        (t_j = fma(z2_j, c2, c1 z1_j), the fine steps' own; both sums rounded once)
// and sqrt(2 dt) z_c = sqrt(dt) W, so the coarse step is heston_step on (W1, T) with the fine walk's c1, c2 and aw and with
// kdt, ktdt and av doubled (exact doublings of the fine walk's rounded constants: `c` below differs from `f` in nothing else).
// The date countdown is shared and counts coarse steps: steps_per_date is even, a date falls after steps_per_date / 2 of them, and
// both legs read the same addend through the same scalar load.
//   ANTI: four walks -- fine and coarse on (z, T), fine and coarse on (-z, -T) -- value = mean of the two differences
// Stream: domain 17, the Heston layout of the FINE walk.
// =========================================================================================
template <class Real>
struct HestonLevelArgs {
    HestonPathArgs<Real> f, c;   // the fine walk (heston_path_kernel's arguments) and the coarse one
};

// what a lane carries per direction: the two legs and their running sums over the dates
template <class Real>
struct HestonLevelSide {
    HestonSide<Real> f, c;
    Real acc_f, acc_c;
};

template <class Real>
__device__ __forceinline__ void heston_level_date(HestonLevelSide<Real> &s, Real addend, const HestonLevelArgs<Real> &o)
{
    heston_date<0>(s.f, s.acc_f, addend, o.f);
    heston_date<0>(s.c, s.acc_c, addend, o.c);
}

template <class Real>
__device__ __forceinline__ Real heston_level_value(const HestonLevelSide<Real> &s, const HestonLevelArgs<Real> &o)
{
    return heston_path_value<0>(s.f, s.acc_f, o.f) - heston_path_value<0>(s.c, s.acc_c, o.c);
}

// fp32: one Philox block = two fine steps = exactly one coarse step; a trip is a block
template <bool ANTI, class Gen>
__device__ __forceinline__ float heston_level_walk(Gen &gen, const HestonLevelArgs<float> &o, const Work &w, uint32_t c0)
{
    constexpr int NPB = Gen::template npb<float>();
    static_assert(NPB == 4, "two fine steps per block");
    const int n = o.f.h.n_steps;   // even
    const HestonSide<float> start = {o.f.h.v0, 0.0f, 0.0f};
    HestonLevelSide<float> p = {start, start, 0.0f, 0.0f}, q = p;
    float z[NPB];
    int d = 0, left = o.c.steps_per_date;
    for (int j = 0; j < n; j += 2) {
        gen.normals(w, c0, (uint32_t)(j >> 1), 17u /*MC_DOMAIN_HESTON_LEVEL*/, z);
        const float ta = __builtin_fmaf(z[1], o.f.h.c2, o.f.h.c1 * z[0]);
        const float tb = __builtin_fmaf(z[3], o.f.h.c2, o.f.h.c1 * z[2]);
        const float W1 = z[0] + z[2], T = ta + tb;
        heston_step(p.f, z[0], ta, o.f.h, 0.0f);
        heston_step(p.f, z[2], tb, o.f.h, 0.0f);
        heston_step(p.c, W1, T, o.c.h, 0.0f);
        if (ANTI) {
            heston_step(q.f, -z[0], -ta, o.f.h, 0.0f);
            heston_step(q.f, -z[2], -tb, o.f.h, 0.0f);
            heston_step(q.c, -W1, -T, o.c.h, 0.0f);
        }
        if (--left == 0) {   // wave-uniform
            const float addend = o.f.tab[d];
            heston_level_date(p, addend, o);
            if (ANTI)
                heston_level_date(q, addend, o);
            ++d;
            left = o.c.steps_per_date;
        }
    }
    float val = heston_level_value(p, o);
    if (ANTI)
        val = 0.5f * (val + heston_level_value(q, o));
    return val;
}

// fp64: heston_path_walk<double>'s trips.  Four pairs = four fine steps = two coarse steps, taken after the second and the fourth
// pair; m = 2 (mod 4) leaves one coarse step, taken on phases 0 and 1 of the cursor (compile-time constants again).
template <bool ANTI, class Gen>
__device__ __forceinline__ double heston_level_walk(Gen &gen, const HestonLevelArgs<double> &o, const Work &w, uint32_t c0)
{
    static_assert(Gen::cursor_phases == 4, "a coarse step is half a trip of the pair cursor");
    const int n = o.f.h.n_steps;   // even
    const HestonSide<double> start = {o.f.h.v0, 0.0, 0.0};
    HestonLevelSide<double> p = {start, start, 0.0, 0.0}, q = p;
    const double floor = 0x1p-1000;
    F64K K;
    K.load();
    typename Gen::Carry carry;
    carry.K = &K;
    double W1 = 0.0, T = 0.0;
    auto fine =[&](double z1, double z2, bool second) {
        const double t = __builtin_fma(z2, o.f.h.c2, o.f.h.c1 * z1);
        heston_step(p.f, z1, t, o.f.h, floor);
        if (ANTI)
            heston_step(q.f, -z1, -t, o.f.h, floor);
        W1 = second ? W1 + z1 : z1;
        T = second ? T + t : t;
    };
    int d = 0, left = o.c.steps_per_date;
    auto coarse = [&]() {
        heston_step(p.c, W1, T, o.c.h, floor);
        if (ANTI)
            heston_step(q.c, -W1, -T, o.c.h, floor);
        if (--left == 0) {   // wave-uniform
            const double addend = o.f.tab[d];
            heston_level_date(p, addend, o);
            if (ANTI)
                heston_level_date(q, addend, o);
            ++d;
            left = o.c.steps_per_date;
        }
    };
    int j = 0;
#pragma unroll 1
    for (; j + 4 <= n; j += 4) {
        uint32_t g4 = (uint32_t)(j >> 2) << 2;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            // heston_path<double>'s tie: a step's generator call starts after the variance of the step before it
            if (ANTI && k)
                asm("" : "+v"(p.f.V), "+s"(g4));
            double z0, z1;
            gen.pair(w, c0, 17u /*MC_DOMAIN_HESTON_LEVEL*/, g4 | k, carry, z0, z1);
            fine(z0, z1, k & 1u);
            if (k & 1u)
                coarse();
        }
    }
    if (j < n) {   // wave-uniform: m = 2 (mod 4), the last coarse step
        uint32_t g4 = (uint32_t)(j >> 2) << 2;
#pragma unroll
        for (uint32_t k = 0; k < 2; ++k) {
            if (ANTI && k)
                asm("" : "+v"(p.f.V), "+s"(g4));
            double z0, z1;
            gen.pair(w, c0, 17u /*MC_DOMAIN_HESTON_LEVEL*/, g4 | k, carry, z0, z1);
            fine(z0, z1, k & 1u);
        }
        coarse();
    }
    gen.pairs_done((uint32_t)n);
    double val = heston_level_value(p, o);
    if (ANTI)
        val = 0.5 * (val + heston_level_value(q, o));
    return val;
}

// one lane per path, grid-stride over the segment's paths
template <class Real, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void heston_level_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const HestonLevelArgs<Real> o, const Work w, Real *__restrict__ out)
{
    stage_tables<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = heston_level_walk<ANTI>(gen, o, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// Calls and puts under a local-volatility surface sigma(t, S): log-Euler on m equal steps (the model is stated in mc_mi355x.h),
// the European (PAYOFF = 0), the arithmetic-average (1) and the single-barrier payoff monitored on the dates (2).  Not in the
// reference.  The lane's state is y = ln(S / S0) in natural-log units (the surface is sampled in them) and the step is
//   u = med3(fma(y, inv_h, u0), 0, n_nodes - 1);  i = min(int(u), n_nodes - 2);  (a, b) = lds[slice + i];  sig = fma(u - i, b, a)
//   y = fma(sig, sdt z, y + fma(sig sig, -dt/2, r dt))
// The first walk here whose table index is the LANE's: every other per-call table is indexed by something wave-uniform and comes
// through scalar loads, this one is a gather.  The surface travels as interleaved (a_i, b_i = a_{i+1} - a_i) pairs (b folded in
// fp64 on the host and rounded once; the last pair of a row has b = 0 and is never read), which the workgroup copies from the
// context's constant table into dynamic LDS sized to this call's surface, once, before the grid-stride loop: a lookup is ONE LDS read
// of 8 bytes (fp32) or 16 bytes (fp64) per direction per step.  The slice is wave-uniform: its base index lives in an SGPR,
// advanced by a scalar countdown of the steps left in it, exactly as the date's countdown (heston_path_walk).  An odd number of
// steps per slice or per date puts a boundary between the steps of a block or a pair: both countdowns run after EVERY step.
//   date:  Asian   acc += E(fma(y, esc, x0)), x0 = ln S0 in exponent units, esc = 1 (f64) or log2 e (f32)
//          barrier mn = min(mn, fma(nsg, y, dk)), dk = sgn ln(B / S0), nsg = -sgn;  P = [mn > 0] by a select
//   value: European / barrier (c0 + c1 P) (phi (E(fma(y, esc, x0)) - K))^+;  Asian (phi (acc inv_m - K))^+;  phi = +-1 in an SGPR
// The date's addend does not depend on the date here (the drift is part of the step), so it is a kernel argument, not a table.
//   ANTI: a second y walked on -z with its own lookups and its own running sum / minimum; value = mean of the two
// Stream: domain 16, step j (0-based here) = entry j % NPB of block j / NPB: the Asian layout.
// =========================================================================================
template <class Real>
struct LocalVolArgs {
    const Real *pairs;       // n_pairs (a, b) pairs, row-major [n_times][n_nodes]
    int n_pairs, n_nodes;
    int n_steps, steps_per_slice, steps_per_date;
    Real inv_h, u0;          // u = clamp(fma(y, inv_h, u0), 0, n_nodes - 1): 1 / h, -y_lo / h
    Real rdt, mhdt, sdt;     // r dt, -dt / 2, sqrt(dt)
    Real x0;                 // S = E(fma(y, esc, x0)), esc = exp_units<Real>()
    Real strike;
    Real inv_m;              // Asian: 1 / n_dates
    Real dk;                 // barrier: d = fma(nsg, y, dk), value = (c0 + c1 P) payoff
    float phi, nsg, c0, c1;  // +-1 and 0: exact in a float, one SGPR each in either precision
};

// the exponential's units per natural-log unit: exp_model is 2^x in fp32
template <class Real> __device__ __forceinline__ constexpr Real exp_units() { return sizeof(Real) == 4 ? (Real)1.4426950408889634074 : (Real)1; }

template <class Real> struct LvPair;
template <> struct LvPair<float> { using type = float2; };
template <> struct LvPair<double> { using type = double2; };

__device__ __forceinline__ float clamp_r(float u, float hi) { return __builtin_amdgcn_fmed3f(u, 0.0f, hi); }
__device__ __forceinline__ double clamp_r(double u, double hi) { return min_f64(max0(u), hi); }

template <class Real>
__device__ __forceinline__ void localvol_step(Real &y, Real zs, const typename LvPair<Real>::type *__restrict__ row, const LocalVolArgs<Real> &o)
{
    const Real u = clamp_r(fma_r(y, o.inv_h, o.u0), (Real)(o.n_nodes - 1));
    int i = (int)u;
    i = i < o.n_nodes - 2 ? i : o.n_nodes - 2;
    const auto ab = row[i];
    const Real sig = fma_r(u - (Real)i, ab.y, ab.x);
    y = fma_r(sig, zs, y + fma_r(sig * sig, o.mhdt, o.rdt));
}

template <int PAYOFF, class Real>
__device__ __forceinline__ void localvol_date(Real y, Real &acc, const LocalVolArgs<Real> &o)
{
    if (PAYOFF == 1)
        acc += exp_model(fma_r(y, exp_units<Real>(), o.x0));
    else
        acc = min_r(acc, fma_r((Real)o.nsg, y, o.dk));
}

template <int PAYOFF, class Real>
__device__ __forceinline__ Real localvol_value(Real y, Real acc, const LocalVolArgs<Real> &o)
{
    const Real level = PAYOFF == 1 ? acc * o.inv_m : exp_model(fma_r(y, exp_units<Real>(), o.x0));
    const Real a = (Real)o.phi * (level - o.strike);
    const Real pay = a > 0 ? a : 0;
    if (PAYOFF != 2)
        return pay;
    const Real P = acc > 0 ? (Real)1 : (Real)0;   // the select, as barrier_value
    return fma_r((Real)o.c1, P, (Real)o.c0) * pay;
}

// The walk of one path.  step(z) is one Euler step of both directions followed by the two scalar countdowns; the trips differ by
// precision: fp32 one Philox block = four steps, then one block for the one to three steps left; fp64 four Box-Muller pairs =
// eight steps (the cursor's phase a compile-time constant in each copy), then one pair per trip, the last of them possibly half used.
template <bool ANTI, int PAYOFF, class Real, class Gen>
__device__ __forceinline__ Real localvol_walk(Gen &gen, const LocalVolArgs<Real> &o, const typename LvPair<Real>::type *__restrict__ lds, const Work &w,
                                              uint32_t c0)
{
    const int n = o.n_steps;
    Real y = 0, y_m = 0;
    Real acc = PAYOFF == 2 ? (Real)__builtin_inf() : (Real)0, acc_m = acc;
    int base = 0, s_left = o.steps_per_slice, d_left = o.steps_per_date;   // wave-uniform: SGPRs
    auto step = [&](Real z) {
        const Real zs = o.sdt * z;
        localvol_step(y, zs, lds + base, o);
        if (ANTI)
            localvol_step(y_m, -zs, lds + base, o);
        if (--s_left == 0) {   // wave-uniform
            base += o.n_nodes;
            s_left = o.steps_per_slice;
        }
        if (PAYOFF != 0 && --d_left == 0) {   // wave-uniform
            localvol_date<PAYOFF>(y, acc, o);
            if (ANTI)
                localvol_date<PAYOFF>(y_m, acc_m, o);
            d_left = o.steps_per_date;
        }
    };
    if constexpr (sizeof(Real) == 4) {
        constexpr int NPB = Gen::template npb<float>();
        static_assert(NPB == 4, "four steps per block");
        float z[NPB];
        int j = 0;
        for (; j + NPB <= n; j += NPB) {
            gen.normals(w, c0, (uint32_t)(j / NPB), 16u /*MC_DOMAIN_LOCALVOL*/, z);
            step(z[0]);
            step(z[1]);
            step(z[2]);
            step(z[3]);
        }
        if (j < n) {   // wave-uniform: one to three steps left
            gen.normals(w, c0, (uint32_t)(j / NPB), 16u /*MC_DOMAIN_LOCALVOL*/, z);
            step(z[0]);
            if (j + 1 < n)
                step(z[1]);
            if (j + 2 < n)
                step(z[2]);
        }
    } else {
        F64K K;
        K.load();
        typename Gen::Carry carry;
        carry.K = &K;
        int j = 0;
        if constexpr (Gen::cursor_phases > 1) {
#pragma unroll 1
            for (; j + 8 <= n; j += 8) {
                uint32_t g4 = (uint32_t)(j >> 3) << 2;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    // heston_path<double>'s tie: a pair's generator call starts after the steps of the pair before it.  Left free, hipcc
                    // overlaps the four calls of a trip and the antithetic European form needs 129 vector registers: three waves per SIMD
                    if (ANTI && k)
                        asm("" : "+v"(y), "+s"(g4));
                    double z0, z1;
                    gen.pair(w, c0, 16u /*MC_DOMAIN_LOCALVOL*/, g4 | k, carry, z0, z1);
                    step(z0);
                    step(z1);
                }
            }
        }
#pragma unroll 1
        for (; j < n; j += 2) {
            double z0, z1;
            gen.pair(w, c0, 16u /*MC_DOMAIN_LOCALVOL*/, (uint32_t)(j >> 1), carry, z0, z1);
            step(z0);
            if (j + 1 < n)   // wave-uniform
                step(z1);
        }
        gen.pairs_done((uint32_t)((n + 1) >> 1));
    }
    Real val = localvol_value<PAYOFF>(y, acc, o);
    if (ANTI)
        val = (Real)0.5 * (val + localvol_value<PAYOFF>(y_m, acc_m, o));
    return val;
}

// one lane per path, grid-stride over the segment's paths; dynamic LDS: n_pairs pairs
template <class Real, bool ANTI, int PAYOFF, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void localvol_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const LocalVolArgs<Real> o, const Work w, Real *__restrict__ out)
{
    using Pair = typename LvPair<Real>::type;
    stage_tables<Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Pair *lds = reinterpret_cast<Pair *>(lds_raw);
    for (int k = threadIdx.x; k < o.n_pairs; k += GROUP)
        lds[k] = reinterpret_cast<const Pair *>(o.pairs)[k];
    __syncthreads();
    const uint32_t stride = gridDim.x * GROUP;
    double acc_s = 0.0, acc_q = 0.0;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        const Real p = localvol_walk<ANTI, PAYOFF, Real>(gen, o, lds, w, w.unit_lo + i);
        acc_s += (double)p;
        acc_q = __builtin_fma((double)p, (double)p, acc_q);
        if (out)  // wave-uniform: per-path dump for the parity tests
            out[i] = p;
    }
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// =========================================================================================
// CVA, parallel in the DATE axis. Reference loop: dp/MonteCarloKernel.cu:241-262 -- one thread walks all N_GRID dates of
// its path.  With the reformulation above the lane's only state is W_j = z_1 + ... + z_j and everything else is a table
// row of the date, so the walk is a prefix sum followed by independent work: here a path's dates are shared by
// L = 2^log2_lanes ADJACENT lanes (L = 2 ... 64).  Per round of CH * L dates, lane `sub` of the path owns the CH dates
// [r0 + sub CH, r0 + (sub + 1) CH):
//   1. it draws ITS dates' normals -- the generator is counter-based (block = date / NPB): nothing is handed over --
//      and keeps them in registers (CH of them);
//   2. one DPP scan over the L lanes (row_shr inside rows of 16, row_bcast across rows: pure VALU) turns the chunk sums into every
//      lane's W offset;
//   3. it prices its CH dates with the same per-date operations as cva_kernel, the table row read per LANE from an LDS copy
//      of the table (the date is no longer wave-uniform, so the scalar loads of cva_kernel are not available);
// and after the last round one DPP reduction over the L lanes forms the path's sum_j dp_j ee_j BEFORE it is squared.  The
// values differ from cva_kernel's only by the association of two sums (W, and the sum over dates): 1e-16-level in fp64.
// What it is for (mc_api.hip: cva_enqueue picks L): a unit of work is 1/L of a path, so
//   * the LAST PARTIAL WAVE-TRIP of a large call (cva_kernel's time is a staircase in steps of 64 lanes x 1024 SIMDs = 65 536
//     paths: 1.25e6 paths -- C5's shard of 8 -- pay 20 trips for 19.07) is priced by date-parallel workgroups of the SAME launch
//     (cva_split_kernel below);
//   * a SMALL call (the reference driver's own 131 072 paths, dp/cvaOpt.cu:12-15: two waves per SIMD) fills the chip
//     (cva_dates_kernel).
// Generators: the counter-based ones and the external array (XORWOW is one sequence per lane: a path cannot be entered in
// the middle).  Grid-stride over path slots; a wave's lanes all run the same number of trips (lanes beyond the range price
// a valid path and contribute nothing), because the scans need every lane.
// =========================================================================================
__device__ __forceinline__ float lane_fetch(float v, uint32_t src_lane)   // v of lane `src_lane` (mod 64)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)(src_lane << 2), __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ double lane_fetch(double v, uint32_t src_lane)
{
    const int lo = __builtin_amdgcn_ds_bpermute((int)(src_lane << 2), __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute((int)(src_lane << 2), __double2hiint(v));
    return __hiloint2double(hi, lo);
}
// DPP moves inside the wave (pure VALU: no LDS round trip on the scan's dependent chain).  Lanes without a source lane, or in a
// row masked off, receive 0.  Controls (gfx9 encoding): row_shr:n = 0x110 + n (shift right by n inside a row of 16),
// wave_shr:1 = 0x138 (the whole wave by one lane); the others are mc_reduce.hpp's.
constexpr int DPP_ROW_SHR = 0x110, DPP_WAVE_SHR1 = 0x138;
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_fetch(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, false));
}
// Inclusive scan of `v` over aligned groups of L = 2^k <= 64 adjacent lanes (`sub` = lane & (L - 1), L wave-uniform): first inside
// the rows of 16 (row_shr 1, 2, 4, 8), then row totals across rows (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3).
template <class Real>
__device__ __forceinline__ Real group_scan_incl(Real v, uint32_t L, uint32_t sub)
{
    const uint32_t r = sub & 15u;   // position inside the row of 16
    if (L > 1) { const Real t = dpp_fetch<DPP_ROW_SHR + 1>(v); v += r >= 1u ? t : (Real)0; }
    if (L > 2) { const Real t = dpp_fetch<DPP_ROW_SHR + 2>(v); v += r >= 2u ? t : (Real)0; }
    if (L > 4) { const Real t = dpp_fetch<DPP_ROW_SHR + 4>(v); v += r >= 4u ? t : (Real)0; }
    if (L > 8) { const Real t = dpp_fetch<DPP_ROW_SHR + 8>(v); v += r >= 8u ? t : (Real)0; }
    if (L > 16) { const Real t = dpp_fetch<DPP_ROW_BCAST15, 0xA>(v); v += (sub & 16u) ? t : (Real)0; }
    if (L > 32) { const Real t = dpp_fetch<DPP_ROW_BCAST31, 0xC>(v); v += (sub & 32u) ? t : (Real)0; }
    return v;
}
// Sum of `v` over the same groups, valid in the group's LAST lane (sub == L - 1; for L <= 16 in every lane of the group).
template <class Real>
__device__ __forceinline__ Real group_total_in_last_lane(Real v, uint32_t L)
{
    if (L > 1) v += dpp_fetch<DPP_QUAD_XOR1>(v);
    if (L > 2) v += dpp_fetch<DPP_QUAD_XOR2>(v);
    if (L > 4) v += dpp_fetch<DPP_ROW_HALF_MIRROR>(v);
    if (L > 8) v += dpp_fetch<DPP_ROW_MIRROR>(v);
    if (L > 16) v += dpp_fetch<DPP_ROW_BCAST15, 0xA>(v);
    if (L > 32) v += dpp_fetch<DPP_ROW_BCAST31, 0xC>(v);
    return v;
}

// exposures of two consecutive dates of one path, table rows in vector registers; same operations per date as the pair
// forms of cva_path (fp32: the two dates in the halves of every packed instruction; fp64: one shared reciprocal)
// fp32: `row` = the pair's 12 floats {g, g', e1, e1', e2, e2', xk, xk', disc, disc', dp, dp'} (date, next date) read per lane from the
// LDS copy -- adjacent registers are ready-made packed operands (two separate 6-float rows made the compiler transpose them
// through scratch memory: 28 bytes per lane and twice the time of the one-lane-per-path kernel)
__device__ __forceinline__ f2 exposure_pair_rows(float bx, f2 Wp, const float (&row)[12])
{
    return bs_exposure_dates(pk_fma(Wp, (f2){bx, bx}, (f2){row[6], row[7]}), Wp, (f2){row[0], row[1]}, (f2){row[2], row[3]}, (f2){row[4], row[5]},
                             (f2){row[8], row[9]});
}
__device__ __forceinline__ void exposure_pair_rows(double bx, double W_a, double W_b, const CvaStep<double> &sa, const CvaStep<double> &sb,
                                                   double &ee_a, double &ee_b)
{
    bs_exposure2<false>(__builtin_fma(W_a, bx, sa.xk), W_a, sa, __builtin_fma(W_b, bx, sb.xk), W_b, sb, ee_a, ee_b);
}
template <class Real>
__device__ __forceinline__ Real intrinsic_exposure(Real bx, Real W, Real xk, Real strike)
{
    const Real iv = exp_model(fma_r(W, bx, xk)) - strike;
    return iv > 0 ? iv : (Real)0;
}

// workgroup `block` of `n_blocks` date-parallel workgroups; lds_raw: room for the per-date table (n_dates rows)
template <class Real, int CH, bool ANTI, class Gen>
__device__ __forceinline__ void cva_dates_role(const CvaArgs<Real> &o, const Work &w, const uint32_t log2_lanes, Real *__restrict__ out, uint32_t block,
                                               uint32_t n_blocks, unsigned char *lds_raw, double &acc_s, double &acc_q)
{
    constexpr int NPB = Gen::template npb<Real>();
    static_assert(CH % NPB == 0 && CH % 2 == 0, "a lane's chunk is whole generator blocks and whole date pairs");
    CvaStep<Real> *rows = reinterpret_cast<CvaStep<Real> *>(lds_raw);
    const int n_dates = o.n_bs + o.last_intrinsic;
    {   // the per-date table, once per workgroup (n_dates * 6 reals, rounded up to whole date pairs; the host checked that it fits).
        // fp64: the rows as they are.  fp32: two dates per row, field by field -- {g, g', e1, e1', ...} -- the packed operands of a pair
        const Real *src = reinterpret_cast<const Real *>(o.steps);
        Real *dst = reinterpret_cast<Real *>(lds_raw);
        for (int k = threadIdx.x; k < 6 * (n_dates + (n_dates & 1)); k += GROUP) {
            const int date = k / 6, field = k - 6 * date;
            const Real x = date < n_dates ? src[k] : (Real)0;
            if constexpr (sizeof(Real) == 4)
                dst[12 * (date >> 1) + 2 * field + (date & 1)] = x;
            else
                dst[k] = x;
        }
    }
    __syncthreads();
    const uint32_t L = 1u << log2_lanes, lane = threadIdx.x & 63u, sub = lane & (L - 1u);
    const uint32_t slots = (uint32_t)GROUP >> log2_lanes;                  // paths a workgroup holds at a time
    const uint32_t stride = n_blocks * slots;
    const uint32_t slot = block * slots + (threadIdx.x >> log2_lanes);
    Gen gen(w);
    for (uint32_t i = slot, i0 = __builtin_amdgcn_readfirstlane(slot); i0 < w.n_units; i += stride, i0 += stride) {   // i0: the wave's first slot
        const bool live = i < w.n_units;
        const uint32_t unit = w.unit_lo + (live ? i : i0);
        Real W_done = 0, acc = 0;   // W_done: the path's W at the end of the previous round
        f2 acc2 = {0.0f, 0.0f};     // fp32: even / odd dates of the packed pairs
        for (int r0 = 0; r0 < n_dates; r0 += CH << log2_lanes) {
            const int j0 = r0 + (int)sub * CH;   // this lane's first date (0-based) of the round: a multiple of CH, so every pair starts on an even date
            Real z[CH];
#pragma unroll
            for (int t = 0; t < CH; ++t)
                z[t] = 0;
            if (j0 < n_dates) {
#pragma unroll
                for (int q = 0; q < CH / NPB; ++q) {
                    Real zz[NPB];
                    gen.normals(w, unit, (uint32_t)(j0 / NPB + q), 3u /*MC_DOMAIN_CVA*/, zz);
#pragma unroll
                    for (int t = 0; t < NPB; ++t)
                        z[q * NPB + t] = (j0 + q * NPB + t < n_dates) ? zz[t] : (Real)0;
                }
            }
            Real incl = z[0];
#pragma unroll
            for (int t = 1; t < CH; ++t)
                incl += z[t];
            incl = group_scan_incl(incl, L, sub);                    // inclusive scan of the chunk sums over the path's L lanes (DPP)
            const Real before = dpp_fetch<DPP_WAVE_SHR1>(incl);      // the lane below's inclusive sum
            Real Wl = sub ? W_done + before : W_done;                 // W at the end of the date before this lane's chunk
            W_done += lane_fetch(incl, lane | (L - 1u));              // the round's total, for the NEXT round: off the dependent chain
#pragma unroll
            for (int t = 0; t < CH; t += 2) {
                const int ja = j0 + t, jb = ja + 1;
                const Real W_a = Wl + z[t], W_b = W_a + z[t + 1];
                Wl = W_b;
                const bool intrinsic_here = o.last_intrinsic && (ja == o.n_bs || jb == o.n_bs);   // one lane of one wave of the path
                if constexpr (sizeof(Real) == 4) {
                    const int pair = (ja < n_dates ? ja : n_dates - 1) >> 1;
                    float row[12];
                    const float *pr = reinterpret_cast<const float *>(lds_raw) + 12 * pair;
#pragma unroll
                    for (int f = 0; f < 12; ++f)
                        row[f] = pr[f];
                    const f2 Wp = {W_a, W_b};
                    f2 ee = exposure_pair_rows(o.bx, Wp, row);
                    if (ANTI)
                        ee += exposure_pair_rows(o.bx, -Wp, row);
                    ee.x = ja < o.n_bs ? ee.x : 0.0f;   // beyond the closed-form dates: the intrinsic-value date below, or nothing
                    ee.y = jb < o.n_bs ? ee.y : 0.0f;
                    if (intrinsic_here) {
                        const bool first = ja == o.n_bs;
                        const float Wi = first ? W_a : W_b, xk = first ? row[6] : row[7];
                        float iv = intrinsic_exposure(o.bx, Wi, xk, o.strike);
                        if (ANTI)
                            iv += intrinsic_exposure(o.bx, -Wi, xk, o.strike);
                        ee.x = first ? iv : ee.x;
                        ee.y = first ? ee.y : iv;
                    }
                    const f2 dp = {ja < n_dates ? row[10] : 0.0f, jb < n_dates ? row[11] : 0.0f};
                    acc2 = pk_fma(dp, ee, acc2);
                } else {
                    const CvaStep<Real> sa = rows[ja < n_dates ? ja : n_dates - 1], sb = rows[jb < n_dates ? jb : n_dates - 1];
                    Real ee_a, ee_b;
                    exposure_pair_rows(o.bx, W_a, W_b, sa, sb, ee_a, ee_b);
                    if (ANTI) {
                        Real em_a, em_b;
                        exposure_pair_rows(o.bx, -W_a, -W_b, sa, sb, em_a, em_b);
                        ee_a += em_a, ee_b += em_b;
                    }
                    ee_a = ja < o.n_bs ? ee_a : (Real)0;   // beyond the closed-form dates: the intrinsic-value date below, or nothing
                    ee_b = jb < o.n_bs ? ee_b : (Real)0;
                    if (intrinsic_here) {
                        const bool first = ja == o.n_bs;
                        const Real Wi = first ? W_a : W_b, xk = first ? sa.xk : sb.xk;
                        Real iv = intrinsic_exposure(o.bx, Wi, xk, o.strike);
                        if (ANTI)
                            iv += intrinsic_exposure(o.bx, -Wi, xk, o.strike);
                        ee_a = first ? iv : ee_a;   // (selects: a reference picked at run time would put both in scratch)
                        ee_b = first ? ee_b : iv;
                    }
                    acc = fma_r(sa.dp, ee_a, acc);
                    acc = fma_r(sb.dp, ee_b, acc);
                }
            }
        }
        if constexpr (sizeof(Real) == 4)
            acc += acc2.x + acc2.y;
        acc = group_total_in_last_lane(acc, L);   // the path's sum over its lanes, in the group's last lane
        const Real p = acc * (ANTI ? o.lgd * (Real)0.5 : o.lgd);
        if (live && sub == L - 1u) {
            acc_s += (double)p;
            acc_q = __builtin_fma((double)p, (double)p, acc_q);
            if (out)
                out[i] = p;
        }
    }
}

template <class Real, int CH, bool ANTI, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void cva_dates_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const CvaArgs<Real> o, const Work w,
                                                          const uint32_t log2_lanes, Real *__restrict__ out)
{
    stage_tables<Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double acc_s = 0.0, acc_q = 0.0;
    cva_dates_role<Real, CH, ANTI, Gen>(o, w, log2_lanes, out, blockIdx.x, gridDim.x, lds_raw, acc_s, acc_q);
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}

// ONE launch for a call that ends in a partial wave-trip: the first `tail_groups` workgroups price the call's last `wt.n_units`
// paths date-parallel, the others the leading whole trips one lane per path.  (Two launches would have to run side by side:
// on one stream the queue's barrier bit serialises them -- gfx950 ignores hipExtAnyOrderLaunch, profiles/r06_any_order_probe.log
// -- and a second stream forked from and joined to the first costs 21-26 us per call whatever the remainder's size,
// half of the trip it saves: profiles/r06_shard_clock_split_two_streams.log.)  The date-parallel workgroups come FIRST in
// the grid: they are dispatched with the first round of the others and are long gone when the last full trip ends.  The
// kernel's registers are the date-parallel role's (fp64: 4 waves per SIMD instead of cva_kernel's 6, which costs cva_kernel's
// loop nothing measurable: profiles/r06_occupancy_probe.log).
template <class Real, int CH, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void cva_split_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const CvaArgs<Real> o, const Work w,
                                                          const Work wt, const uint32_t tail_groups, const uint32_t log2_lanes,
                                                          Real *__restrict__ out, Real *__restrict__ out_tail)
{
    stage_tables<Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double acc_s = 0.0, acc_q = 0.0;
    if (blockIdx.x < tail_groups)   // workgroup-uniform
        cva_dates_role<Real, CH, false, Gen>(o, wt, log2_lanes, out_tail, blockIdx.x, tail_groups, lds_raw, acc_s, acc_q);
    else
        cva_paths_role<Real, false, Gen>(o, w, out, blockIdx.x - tail_groups, gridDim.x - tail_groups, lds_raw, acc_s, acc_q);
    group_sum2(acc_s, acc_q);
    finish_group(acc_s, acc_q);
}


// =========================================================================================
// Greeks of the basket call (the reference prices only).  Per path, in the reference's own (unfolded) device
// formulas dp/MonteCarloKernel.cu:74-101 on the pricing kernels' normals:
//     bt_a = sum_{b<=a} L_ab g_b + d_a,   s_a = S_a exp(mu_a + v_a bt_a sqrt T),   B = sum_a w_a s_a,   I = [B > K]
// PATHWISE (LR = false):
//     payoff = I (B - K),   d payoff / d S_a = I w_a s_a / S_a,   d payoff / d v_a = I w_a s_a (bt_a sqrt T - v_a T)
// LIKELIHOOD RATIO (LR = true): the payoff times the score of the terminal prices' joint lognormal density.  With
// x = ln S(T) ~ N(m, Sigma), Sigma = T D L L' D, D = diag(v), the whitened vector y = L^-T g (y_a = sum_{b>=a} M_ab g_b,
// M = L^-T on the host) gives Sigma^-1 (x - m) = D^-1 y / sqrt T and
//     score_{S_a} = y_a / (S_a v_a sqrt T),
//     score_{v_a} = (y_a (L g)_a - 1) / v_a + (sqrt T d_a - v_a T) y_a / (v_a sqrt T)
// (one asset: z / (S sigma sqrt T) and (z^2 - 1) / sigma - z sqrt T, the vanilla kernel's).  No indicator is differentiated;
// needs a non-singular factor (every L_aa > 0).
// ONE PASS per BASKET_GREEKS_CHUNK assets: a lane keeps the (sum, sum2) pairs of the price and of the two derivatives of the
// A = 8 assets of its workgroup's chunk (grid y index) in registers -- 2 + 4 A doubles -- so a basket of n assets is simulated
// ceil(n / 8) times instead of n times (round 5: one pass per asset; n = 16: profiles/r06_basket_greeks_one_pass.log).  Generic
// in n (normals in the lane's LDS column, constants through scalar loads).  Planes of the pair buffer:
// 0 = price (published by y = 0 only), 1 + a = delta_a, 1 + n + a = vega_a.
// Constant table (Real): L[n*n] row-major | d[n] | mu[n] | v[n] | w[n] | s[n] | inv_s[n] | vt[n] (= v_a T)
//                        | LR only: M[n*n] | inv_svt[n] (= 1 / (S_a v_a sqrt T)) | inv_v[n] | mcoef[n] (= (sqrt T d_a - v_a T) / (v_a sqrt T)).
// =========================================================================================
template <class Real>
struct BasketGreeks {
    const Real *consts;
    int n;
    Real strike, sqrt_t;
};
#ifndef MC_BASKET_GREEKS_CHUNK
#define MC_BASKET_GREEKS_CHUNK 8   // -DMC_BASKET_GREEKS_CHUNK=1 rebuilds round 5's one pass per asset (the A/B of profiles/r06_basket_greeks_one_pass.log)
#endif
constexpr int BASKET_GREEKS_CHUNK = MC_BASKET_GREEKS_CHUNK;

__device__ __forceinline__ float exp_nat(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ double exp_nat(double x) { return exp_f64(x); }

// What basket_greeks_kernel and basket_gamma_kernel share: the constant table's arrays (scalar loads; M .. mcoef in the LR table
// only) and the staging of a path's normals into the lane's LDS column.  The loops over the assets stay in the kernels: moved into
// a helper, a loop whose trip count is only known at run time is optimised before it is inlined and compiles to different code.
template <class Real>
struct BasketTable {
    typedef const __attribute__((address_space(4))) Real *cptr;
    static constexpr int NPB = GenPhilox::npb<Real>();
    int n, nblk;   // assets, blocks of NPB normals per path
    cptr L, d, mu, v, wt, s0, inv_s, vt, M, inv_svt, inv_v, mcoef;
    __device__ __forceinline__ BasketTable(const BasketGreeks<Real> &o)
        : n(o.n), nblk((o.n + NPB - 1) / NPB), L((cptr)o.consts), d(L + n * n), mu(d + n), v(mu + n), wt(v + n), s0(wt + n),
          inv_s(s0 + n), vt(inv_s + n), M(vt + n), inv_svt(M + n * n), inv_v(inv_svt + n), mcoef(inv_v + n) {}

    // block b of the unit's normals into the lane's column g (stride GROUP): assets b NPB ..
    __device__ __forceinline__ void stage(GenPhilox &gen, const Work &w, uint32_t unit, int b, Real *g) const
    {
        Real z[NPB];
        gen.normals(w, unit, (uint32_t)b, 2u /*MC_DOMAIN_BASKET*/, z);
#pragma unroll
        for (int j = 0; j < NPB; ++j)
            g[(b * NPB + j) * GROUP] = z[j];
    }
};

template <class Real, bool LR>
__global__ __launch_bounds__(GROUP) void basket_greeks_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const BasketGreeks<Real> o, const Work w)
{
    constexpr int A = BASKET_GREEKS_CHUNK;
    stage_tables<Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Real *g = reinterpret_cast<Real *>(lds_raw) + threadIdx.x;  // this lane's column, stride GROUP
    const BasketTable<Real> tb(o);
    const int n = tb.n, chunk = blockIdx.y, a0 = chunk * A;
    GenPhilox gen(w);
    const uint32_t stride = gridDim.x * GROUP;
    double acc[2 + 4 * A];   // pairs: price, then delta and vega of the chunk's asset a0 + k (1 + 2 k, 2 + 2 k)
#pragma unroll
    for (int q = 0; q < 2 + 4 * A; ++q)
        acc[q] = 0;
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        for (int b = 0; b < tb.nblk; ++b)
            tb.stage(gen, w, w.unit_lo + i, b, g);
        Real basket = 0, term[A], bts[A];
#pragma unroll
        for (int k = 0; k < A; ++k)
            term[k] = bts[k] = 0;
        for (int c = 0; c * A < n; ++c) {
#pragma unroll
            for (int k = 0; k < A; ++k) {
                const int a = c * A + k;
                if (a < n) {   // workgroup-uniform
                    Real bt = 0;
                    for (int b = 0; b <= a; ++b)
                        bt = fma_r(tb.L[a * n + b], g[b * GROUP], bt);
                    const Real bt0 = bt;   // (L g)_a, before the drift
                    bt += tb.d[a];
                    const Real t_a = tb.s0[a] * exp_nat(fma_r(tb.v[a] * bt, o.sqrt_t, tb.mu[a])) * tb.wt[a];
                    basket += t_a;
                    if (c == chunk) {   // workgroup-uniform: the assets whose derivatives this workgroup accumulates
                        term[k] = t_a;
                        bts[k] = LR ? bt0 : bt;
                    }
                }
            }
        }
        const bool itm = basket > o.strike;
        const Real payoff = itm ? basket - o.strike : (Real)0;
        pair_add(acc, 0, (double)payoff);
#pragma unroll
        for (int k = 0; k < A; ++k) {
            const int a = a0 + k;
            if (a < n) {   // workgroup-uniform
                double dl, vg;
                if constexpr (LR) {
                    Real y = 0;
                    for (int b = a; b < n; ++b)
                        y = fma_r(tb.M[a * n + b], g[b * GROUP], y);
                    dl = (double)(payoff * (y * tb.inv_svt[a]));
                    vg = (double)(payoff * fma_r(fma_r(y, bts[k], (Real)-1), tb.inv_v[a], tb.mcoef[a] * y));
                } else {
                    dl = itm ? (double)(term[k] * tb.inv_s[a]) : 0.0;
                    vg = itm ? (double)(term[k] * (bts[k] * o.sqrt_t - tb.vt[a])) : 0.0;
                }
                pair_add(acc, 1 + 2 * k, dl);
                pair_add(acc, 2 + 2 * k, vg);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 1 + 2 * A; ++q)
        group_sum2(acc[2 * q], acc[2 * q + 1]);
    const tail_ptr t = late_tail(acc[0]);
    if (chunk == 0)
        pair_publish(t, acc, 0, 0);
#pragma unroll
    for (int k = 0; k < A; ++k)
        if (a0 + k < n) {
            pair_publish(t, acc, 1 + 2 * k, 1 + a0 + k);
            pair_publish(t, acc, 2 + 2 * k, 1 + n + a0 + k);
        }
    arrive_and_finish(t);
}

// =========================================================================================
// Gamma matrix of the basket call by the mixed estimator (the likelihood-ratio derivative of the pathwise delta): with
// p_a = I w_a S_a(T) / S_a (the pathwise delta term), y = L^-T g and c_b = 1 / (S_b v_b sqrt T) (inv_svt, the LR delta score),
//     G_ab = 1/2 (p_a y_b c_b + p_b y_a c_a) - [a == b] p_a / S_a
// (one asset: the vanilla kernel's gamma).  The n (n + 1) / 2 entries a <= b are cut into BASKET_GAMMA_TILE^2 tiles of the upper
// triangle; the grid's y index is the tile and each workgroup simulates the paths once for its tile (rows ti T.., columns
// tj T..), keeping one (sum, sum2) pair per entry in registers: 2 T^2 = 32 doubles at T = 4, the budget of basket_greeks_kernel's
// 8-asset chunk.  Planes: 0 = price (published by tile 0 only, the same bits as basket_greeks_kernel's), 1 + u(a, b) the
// upper-triangle entry in row-major order, u(a, b) = a n - a (a - 1) / 2 + b - a.  Constant table: basket_greeks_kernel's LR one.
// =========================================================================================
constexpr int BASKET_GAMMA_TILE = 4;

template <class Real>
__global__ __launch_bounds__(GROUP) void basket_gamma_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const BasketGreeks<Real> o, const Work w)
{
    constexpr int T = BASKET_GAMMA_TILE;
    stage_tables<Real>();
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Real *g = reinterpret_cast<Real *>(lds_raw) + threadIdx.x;  // this lane's column, stride GROUP
    const int n = o.n, nt = (n + T - 1) / T;
    int ti = 0, rem = (int)blockIdx.y;   // tile -> (row tile ti, column tile tj >= ti), workgroup-uniform
    while (rem >= nt - ti)
        rem -= nt - ti, ++ti;
    const int tj = ti + rem, a0 = ti * T, b0 = tj * T;
    GenPhilox gen(w);
    const BasketTable<Real> tb(o);
    const uint32_t stride = gridDim.x * GROUP;
    double acc[2 + 2 * T * T];   // pairs: price, then entry (a0 + r, b0 + k) in 1 + r T + k
#pragma unroll
    for (int q = 0; q < 2 + 2 * T * T; ++q)
        acc[q] = 0;
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        for (int b = 0; b < tb.nblk; ++b)
            tb.stage(gen, w, w.unit_lo + i, b, g);
        Real basket = 0, tr[T], tc[T];
#pragma unroll
        for (int k = 0; k < T; ++k)
            tr[k] = tc[k] = 0;
        for (int c = 0; c * T < n; ++c) {
#pragma unroll
            for (int k = 0; k < T; ++k) {
                const int a = c * T + k;
                if (a < n) {   // workgroup-uniform
                    Real bt = 0;
                    for (int b = 0; b <= a; ++b)
                        bt = fma_r(tb.L[a * n + b], g[b * GROUP], bt);
                    bt += tb.d[a];
                    const Real t_a = tb.s0[a] * exp_nat(fma_r(tb.v[a] * bt, o.sqrt_t, tb.mu[a])) * tb.wt[a];
                    basket += t_a;
                    if (c == ti)   // workgroup-uniform: the tile's row and column assets
                        tr[k] = t_a;
                    if (c == tj)
                        tc[k] = t_a;
                }
            }
        }
        const bool itm = basket > o.strike;
        const Real payoff = itm ? basket - o.strike : (Real)0;
        pair_add(acc, 0, (double)payoff);
        // p and the LR delta score q = y c of the tile's rows (r) and columns (c)
        Real pr[T], qr[T], pc[T], qc[T];
#pragma unroll
        for (int k = 0; k < T; ++k) {
            pr[k] = qr[k] = pc[k] = qc[k] = 0;
            const int a = a0 + k, b = b0 + k;
            if (a < n) {   // workgroup-uniform
                Real y = 0;
                for (int e = a; e < n; ++e)
                    y = fma_r(tb.M[a * n + e], g[e * GROUP], y);
                pr[k] = itm ? tr[k] * tb.inv_s[a] : (Real)0;
                qr[k] = y * tb.inv_svt[a];
            }
            if (b < n) {
                Real y = 0;
                for (int e = b; e < n; ++e)
                    y = fma_r(tb.M[b * n + e], g[e * GROUP], y);
                pc[k] = itm ? tc[k] * tb.inv_s[b] : (Real)0;
                qc[k] = y * tb.inv_svt[b];
            }
        }
#pragma unroll
        for (int r = 0; r < T; ++r)
#pragma unroll
            for (int k = 0; k < T; ++k) {
                const int a = a0 + r, b = b0 + k;
                if (a <= b && b < n) {   // workgroup-uniform
                    Real e = (Real)0.5 * fma_r(pr[r], qc[k], pc[k] * qr[r]);
                    if (a == b)
                        e = fma_r(-pr[r], tb.inv_s[a], e);
                    pair_add(acc, 1 + r * T + k, (double)e);
                }
            }
    }
#pragma unroll
    for (int q = 0; q < 1 + T * T; ++q)
        group_sum2(acc[2 * q], acc[2 * q + 1]);
    const tail_ptr t = late_tail(acc[0]);
    if (blockIdx.y == 0)
        pair_publish(t, acc, 0, 0);
#pragma unroll
    for (int r = 0; r < T; ++r)
#pragma unroll
        for (int k = 0; k < T; ++k) {
            const int a = a0 + r, b = b0 + k;
            if (a <= b && b < n)
                pair_publish(t, acc, 1 + r * T + k, 1 + a * n - a * (a - 1) / 2 + b - a);
        }
    arrive_and_finish(t);
}

// =========================================================================================
// CVA with its pathwise delta.  CVA = LGD sum_j dp_j C(S_j, tau_j) and S_j is proportional to S_0, so
//     d CVA / d S_0 = LGD sum_j dp_j Delta_j S_j / S_0,   Delta_j = cnd(d1_j)   (I[S_j > K] on an intrinsic-value date)
// and S_j cnd(d1_j) is the first term of the exposure the pricing kernel computes anyway.  Vega: sigma moves the closed
// form (Black-Scholes vega S phi(d1) sqrt(tau) = A sqrt(tau), A being the shared exponential of bs_exposure) and the
// path (d S_j / d sigma = S_j (W_j sqrt(dt) - sigma t_j)):
//     d CVA / d sigma = LGD sum_j dp_j [ A_j sqrt(tau_j) + S_j cnd(d1_j) (W_j sqrt(dt) - sigma t_j) ]
// Plain estimator, one date at a time (a secondary kernel); planes of the pair buffer: 0 = CVA, 1 = delta, 2 = vega.
// =========================================================================================
__device__ __forceinline__ void bs_exposure_delta(float ln2_spot, float W, const CvaStep<float> &st, float &ee, float &s_delta, float &s_phi)
{
    const float spot = __builtin_amdgcn_exp2f(ln2_spot);
    const float d1 = __builtin_fmaf(W, st.g, st.e1), d2 = __builtin_fmaf(W, st.g, st.e2);
    const float A = 0.3989422804014327f * __builtin_amdgcn_exp2f(__builtin_fmaf(d1 * -0.72134752044448170f, d1, ln2_spot));
    const float k1 = __builtin_amdgcn_rcpf(__builtin_fmaf(0.2316419f, fabsf(d1), 1.0f));
    const float k2 = __builtin_amdgcn_rcpf(__builtin_fmaf(0.2316419f, fabsf(d2), 1.0f));
    const float t1 = A * (k1 * (0.31938153f + k1 * (-0.356563782f + k1 * (1.781477937f + k1 * (-1.821255978f + k1 * 1.330274429f)))));
    const float t2 = A * (k2 * (0.31938153f + k2 * (-0.356563782f + k2 * (1.781477937f + k2 * (-1.821255978f + k2 * 1.330274429f)))));
    s_delta = d1 > 0 ? spot - t1 : t1;            // S cnd(d1)
    ee = s_delta - (d2 > 0 ? st.disc - t2 : t2);  // - K e^{-r tau} cnd(d2)
    s_phi = A;                                    // S phi(d1)
}
__device__ __forceinline__ void bs_exposure_delta(double ln_spot, double W, const CvaStep<double> &st, double &ee, double &s_delta, double &s_phi)
{
    const double spot = exp_f64(ln_spot);
    const double d1 = __builtin_fma(W, st.g, st.e1), d2 = __builtin_fma(W, st.g, st.e2);
    const double A = 0.39894228040143267793994605993438 * exp_f64(fmax(__builtin_fma(-0.5 * d1, d1, ln_spot), -800.0));
    double k1, k2;
    recip2_pos(__builtin_fma(0.2316419, fabs(d1), 1.0), __builtin_fma(0.2316419, fabs(d2), 1.0), k1, k2);
    const double t1 = A * hastings_poly(k1), t2 = A * hastings_poly(k2);
    s_delta = d1 > 0 ? spot - t1 : t1;
    ee = s_delta - (d2 > 0 ? st.disc - t2 : t2);
    s_phi = A;
}

// LR = true: the likelihood-ratio forms on the same stream.  Only the first transition's density depends on S_0, every
// transition's on sigma, and the closed-form exposure depends on sigma explicitly (its own vega stays pathwise):
//     d CVA / d S_0   = E[ CVA_path z_1 ] / (S_0 sigma sqrt(dt))
//     d CVA / d sigma = E[ LGD sum_j dp_j S_j phi(d1_j) sqrt(tau_j)  +  CVA_path sum_j ((z_j^2 - 1) / sigma - z_j sqrt(dt)) ]
// (the sums over the dates that draw a normal).  lr_delta = 1 / (S_0 sigma sqrt(dt)), inv_sigma = 1 / sigma.
template <class Real, bool LR>
__global__ __launch_bounds__(GROUP) void cva_greeks_kernel(const Tail /* first argument, read late: mc_reduce.hpp */, const CvaArgs<Real> o, const Work w, Real inv_spot,
                                                           Real sqrt_dt, Real lr_delta, Real inv_sigma)
{
    stage_tables<Real>();
    constexpr int NPB = GenPhilox::npb<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    const int n_dates = o.n_bs + o.last_intrinsic;
    GenPhilox gen(w);
    typedef const __attribute__((address_space(4))) Real *cptr;
    const cptr sqrt_tau = (cptr)o.extra, sig_t = sqrt_tau + n_dates;
    double acc[6] = {};
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        Real W = 0, cva = 0, delta = 0, vega = 0, score = 0, z_first = 0, z[NPB];
        for (int j = 0; j < n_dates; ++j) {   // wave-uniform: table rows through scalar loads
            if (j % NPB == 0)
                gen.normals(w, w.unit_lo + i, (uint32_t)(j / NPB), 3u /*MC_DOMAIN_CVA*/, z);
            const CvaStep<Real> st = o.steps[j];
            Real zz = z[0];
#pragma unroll
            for (int q = 1; q < NPB; ++q)
                zz = (j % NPB == q) ? z[q] : zz;
            W += zz;
            if (LR) {
                z_first = j == 0 ? zz : z_first;
                score += fma_r(fma_r(zz, zz, (Real)-1), inv_sigma, -zz * sqrt_dt);
            }
            const Real ln_spot = fma_r(W, o.bx, st.xk);
            Real ee, sd, sphi;
            if (j < o.n_bs) {
                bs_exposure_delta(ln_spot, W, st, ee, sd, sphi);
            } else {   // residual maturity exactly 0: intrinsic value, derivative I[S > K] S, no closed-form vega
                const Real spot = exp_model(ln_spot);
                const bool itm = spot > o.strike;
                ee = itm ? spot - o.strike : (Real)0;
                sd = itm ? spot : (Real)0;
                sphi = 0;
            }
            cva = fma_r(st.dp, ee, cva);
            if (LR) {
                vega = fma_r(st.dp, sphi * sqrt_tau[j], vega);
            } else {
                delta = fma_r(st.dp, sd, delta);
                vega = fma_r(st.dp, fma_r(sphi, sqrt_tau[j], sd * fma_r(W, sqrt_dt, -sig_t[j])), vega);
            }
        }
        const Real cva_path = cva * o.lgd;
        const double c = (double)cva_path;
        const double dl = LR ? (double)(cva_path * (z_first * lr_delta)) : (double)(delta * o.lgd * inv_spot);
        const double vg = LR ? (double)fma_r(cva_path, score, vega * o.lgd) : (double)(vega * o.lgd);
        pair_add(acc, 0, c);
        pair_add(acc, 1, dl);
        pair_add(acc, 2, vg);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
        group_sum2(acc[2 * q], acc[2 * q + 1]);
    const tail_ptr t = late_tail(acc[0]);
#pragma unroll
    for (int q = 0; q < 3; ++q)
        pair_publish(t, acc, q, q);
    arrive_and_finish(t);
}

// =========================================================================================
// Normals dump (parity tests of the generator itself): Gen::npb<Real>() normals per unit, unit-major.
// =========================================================================================
template <class Real, class Gen = GenPhilox>
__global__ __launch_bounds__(GROUP) void normals_kernel(const Work w, uint32_t block, uint32_t domain,
                                                        Real *__restrict__ out)
{
    stage_tables<Real>();
    constexpr int NPB = Gen::template npb<Real>();
    const uint32_t stride = gridDim.x * GROUP;
    Gen gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride) {
        Real z[NPB];
        gen.normals(w, w.unit_lo + i, block, domain, z);
#pragma unroll
        for (int j = 0; j < NPB; ++j)
            out[(uint64_t)i * NPB + j] = z[j];
    }
}

// =========================================================================================
// Math probe (test hook mc_math_probe, include/mc_mi355x_test.h): the inline functions of mc_math_f64.hpp and the words-to-normals
// steps of mc_rng.hpp -- the functions themselves, as every kernel above calls them -- on caller-chosen inputs.  Item i (PROBE_IN
// 64-bit words in, PROBE_OUT out; doubles as bit patterns, 32-bit values zero-extended) runs on lane i mod 256, so neighbouring
// lanes read different table rows.  `op` is wave-uniform: the numbers are the MC_PROBE_* of the header.
// =========================================================================================
constexpr int PROBE_IN = 4, PROBE_OUT = 8;
__global__ __launch_bounds__(GROUP) void math_probe_kernel(int op, uint32_t n, const uint64_t *__restrict__ in, uint64_t *__restrict__ out)
{
    stage_f64_tables();
    F64K K;
    K.load();
    const auto dbl = [](uint64_t b) { return __longlong_as_double((long long)b); };
    const auto bits = [](double d) { return (uint64_t)__double_as_longlong(d); };
    const auto fbits = [](float f) { return (uint64_t)__float_as_uint(f); };
    const uint32_t stride = gridDim.x * GROUP;
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < n; i += stride) {
        const uint64_t *x = in + (uint64_t)i * PROBE_IN;
        uint64_t *y = out + (uint64_t)i * PROBE_OUT;
        uint64_t r[PROBE_OUT] = {0, 0, 0, 0, 0, 0, 0, 0};
        switch (op) {
        case 0:   // MC_PROBE_NEG2LOG
            r[0] = bits(neg2log_unit_tab(dbl(x[0])));
            r[1] = bits(neg2log_unit_tab(dbl(x[0]), K));
            break;
        case 1: {   // MC_PROBE_SINCOS
            double s, c;
            sincos_turns_tab((uint32_t)x[0], (uint32_t)x[1], s, c);
            r[0] = bits(s), r[1] = bits(c);
            sincos_turns_tab((uint32_t)x[0], (uint32_t)x[1], K, s, c);
            r[2] = bits(s), r[3] = bits(c);
            break;
        }
        case 2:   // MC_PROBE_EXP
            r[0] = bits(exp_f64(dbl(x[0])));
            break;
        case 3:   // MC_PROBE_SQRT
            r[0] = bits(sqrt_pos(dbl(x[0])));
            break;
        case 4: {   // MC_PROBE_RECIP
            const double a1 = dbl(x[0]), a2 = dbl(x[1]), b1 = dbl(x[2]), b2 = dbl(x[3]);
            double q[6];
            r[0] = bits(recip_pos(a1));
            recip2_pos(a1, a2, q[0], q[1]);
            recip4_pos(a1, a2, b1, b2, q[2], q[3], q[4], q[5]);
#pragma unroll
            for (int j = 0; j < 6; ++j)
                r[1 + j] = bits(q[j]);
            break;
        }
        case 5:   // MC_PROBE_U01
            r[0] = bits(u01_f64((uint32_t)x[0], (uint32_t)x[1]));
            break;
        case 6: {   // MC_PROBE_PAIR
            double zc, zs;
            pair_normals_f64((uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2], zc, zs);
            r[0] = bits(zc), r[1] = bits(zs);
            pair_normals_f64((uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2], K, zc, zs);
            r[2] = bits(zc), r[3] = bits(zs);
            break;
        }
        default: {   // MC_PROBE_F32_BLOCK
            const u32x4 w = {(uint32_t)x[0], (uint32_t)x[1], (uint32_t)x[2], (uint32_t)x[3]};
            float z[4];
            words_to_normals(w, z);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                r[j] = fbits(z[j]);
            r[4] = fbits(u01_f32(w.x)), r[5] = fbits(angle_f32(w.y)), r[6] = fbits(u01_f32(w.z)), r[7] = fbits(angle_f32(w.w));
            break;
        }
        }
#pragma unroll
        for (int j = 0; j < PROBE_OUT; ++j)
            y[j] = r[j];
    }
}

// Raw words dump (the tests rebuild the bridge uniforms from them): Philox blocks first_block .. first_block + n_blocks - 1 of
// each unit, four words per block, unit-major: out[(i * n_blocks + b) * 4 + k].
__global__ __launch_bounds__(GROUP) void words_kernel(const Work w, uint32_t domain, uint32_t first_block, uint32_t n_blocks, uint32_t *__restrict__ out)
{
    const uint32_t stride = gridDim.x * GROUP;
    GenPhilox gen(w);
    for (uint32_t i = blockIdx.x * GROUP + threadIdx.x; i < w.n_units; i += stride)
        for (uint32_t b = 0; b < n_blocks; ++b) {
            const u32x4 r = gen.words(w, w.unit_lo + i, first_block + b, domain);
            uint32_t *p = out + ((uint64_t)i * n_blocks + b) * 4u;
            p[0] = r.x, p[1] = r.y, p[2] = r.z, p[3] = r.w;
        }
}

}  // namespace mc
